// The general rows of the QP's full slot form, once per phase (ihm2_amd/csrc/kernels_qp.hip: general_rows, row_dot_full; the packing and the
// reach statement in ihm2_amd/csrc/qp_lds.hpp), on the CPU: the reference's rows at N = 40 -- the one table the form takes -- and at N = 2,
// laid out through the functions api.hip calls, every entry packed by qp_full_slot_pack:
//   * a general-row slot's tile offset is in [0, 16 N), equal to 8 (2 k + row), and no two rows share one;
//   * a box entry is what the kernel packed before the tile existed (restated below), and both kinds keep their word of cf and gam;
//   * the reach statement holds (for N = 2 .. 64), every word a slot reads is one the pass writes, and the words the factor sweep parks in
//     are either rewritten by the pass or read by nobody;
//   * the pass and the one-word read replayed on doubles give, slot by slot, the bits of the chain the form evaluated per slot before.
// Build: g++ -std=c++17 -fsanitize=address,undefined -I ihm2_amd/csrc tools/probes/check_qp_general_rows.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "qp_catalogue.hpp"
#include "qp_lds.hpp"
#include "qp_tables.hpp"

using namespace ihm2;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; if (fails < 50) { std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }

// the reference's bounds at the horizon N (tools/probes/check_full_table.cpp: reference_rows)
static SlotTable reference_table(int N)
{
    const int NS = N + 1;
    std::vector<double> lbx(NS * 8, -1e20), ubx(NS * 8, 1e20), lbu(N * 2), ubu(N * 2), lg(N * 2), ug(N * 2);
    const double lo[8] = {-50.0, -2.0, -0.9, 0.0, -4.0, -4.0, -500.0, -0.5}, hi[8] = {1e4, 2.0, 0.9, 31.0, 4.0, 4.0, 500.0, 0.5};
    const int stage[4] = {1, 3, 6, 7}, terminal[4] = {1, 3, 4, 5};
    for (int k = 1; k <= N; k++)
        for (int q = 0; q < 4; q++) {
            const int i = (k < N) ? stage[q] : terminal[q];
            lbx[k * 8 + i] = lo[i]; ubx[k * 8 + i] = hi[i];
        }
    for (int k = 0; k < N; k++) {
        lbu[k * 2] = -500.0; ubu[k * 2] = 500.0; lbu[k * 2 + 1] = -0.5; ubu[k * 2 + 1] = 0.5;
        lg[k * 2] = -5.0; ug[k * 2] = 5.0; lg[k * 2 + 1] = -0.02; ug[k * 2 + 1] = 0.02;
    }
    ConstraintRows r(NS);
    r.set_box_rows(lbx.data(), ubx.data(), lbu.data(), ubu.data(), lg.data(), ug.data());
    r.set_track_rows(false, nullptr, nullptr);
    return lay_out_slots(r, slot_limits(0));
}

// what the kernel packed for a box row before this form (bits 16..29: 8 (k 10 + c))
static int box_entry_before(int k, int c, int nck) { return ((k * nck + c) * 8) | ((k * 10 + c) << 19); }

static void check_table(int N)
{
    constexpr int NCK = 12;
    const QpLds l = qp_lds(N, qp_lds_class(0, true));
    const SlotTable t = reference_table(N);
    CHECK(t.fit && t.nsoft == 0, "N = %d: the reference's rows fit an all-hard instantiation", N);
    if (N == 40) CHECK(slot_table_full(t, full_form_nslot()), "the reference's table at N = 40 is full");
    CHECK(qp_general_rows_inside(l, N), "N = %d: the reach statement", N);
    const QpReach reach = qp_reach_general_rows(l, N), park = qp_reach_plain_parking(l);
    CHECK(reach.lo == l.tile && reach.hi - reach.lo == 2 * N && reach.hi <= l.tile.end(), "N = %d: the pass writes the first 2 N words of the tile", N);

    std::set<int> offsets, rows;
    int general = 0, boxes = 0;
    std::vector<int> packed;
    for (size_t e = 0; e < t.entries(); e++) {
        if (t.kc[e] < 0) continue;      // padding (no full table has any)
        const int k = t.kc[e] >> 4, c = t.kc[e] & 15, pk = qp_full_slot_pack(k, c, NCK);
        packed.push_back(t.kc[e]);
        CHECK(qp_full_slot_word(pk) == 8 * (k * NCK + c), "slot (%d, %d): its word of cf and gam", k, c);
        if (c >= 10) {
            general++;
            const int off = qp_full_slot_read(pk);
            CHECK(qp_full_slot_general(pk), "slot (%d, %d) is a general row", k, c);
            CHECK(k < N, "slot (%d, %d): no general row on the terminal stage", k, c);
            CHECK(off >= 0 && off < 16 * N, "slot (%d, %d): tile offset %d outside [0, %d)", k, c, off, 16 * N);
            CHECK(off == 8 * (2 * k + (c - 10)), "slot (%d, %d): tile offset %d", k, c, off);
            CHECK(off % 8 == 0 && reach.lo + off / 8 >= reach.lo && reach.lo + off / 8 < reach.hi, "slot (%d, %d) reads a word the pass does not write", k, c);
            CHECK((((unsigned)pk >> 30) & 1) == (unsigned)(c - 10), "slot (%d, %d): which of the two rows", k, c);
            CHECK(offsets.insert(off).second && rows.insert(k * 2 + c - 10).second, "slot (%d, %d): tile offset %d taken twice", k, c, off);
        } else {
            boxes++;
            CHECK(pk == box_entry_before(k, c, NCK), "box (%d, %d): entry %#x, before %#x", k, c, pk, box_entry_before(k, c, NCK));
            CHECK(!qp_full_slot_general(pk) && qp_full_slot_read(pk) == 8 * (k * 10 + c), "box (%d, %d): its word of v", k, c);
        }
    }
    CHECK(general == 2 * N && (int)offsets.size() == 2 * N, "N = %d: %d general-row slots", N, general);
    // the parking words of the factor sweep: below 2 N rewritten by the pass, from 2 N on read by no slot
    for (int w = park.lo; w < park.hi; w++) {
        const bool rewritten = w >= reach.lo && w < reach.hi, read = offsets.count(8 * (w - l.tile)) != 0;
        CHECK(rewritten || !read, "N = %d: tile word %d is parked in, read and not rewritten", N, w - l.tile);
    }

    // ---- the pass and the read on doubles, against the chain per slot ----
    std::mt19937_64 rng(7 + N);
    std::uniform_real_distribution<double> uni(-2.0, 2.0);
    std::vector<double> cd(20), v((N + 1) * 10), tile(QP_TILE_WORDS);
    for (int trial = 0; trial < 3; trial++) {
        for (double &x : cd) x = uni(rng);
        for (double &x : v) x = uni(rng) * std::exp(10.0 * uni(rng));
        if (trial == 1) v[(N / 2) * 10 + 3] = std::nan("0x77");          // a NaN in one stage reaches its two rows and no other
        if (trial == 2) v[5] = INFINITY;
        for (double &x : tile) x = std::nan("0xdead");                  // what the factor sweep may have parked
        for (int e = 0; e < 2 * N; e++) {                                // the pass: element e = 2 k + row
            double acc = 0.0;
            for (int j = 0; j < 10; j++) acc = std::fma(cd[(e & 1) * 10 + j], v[(e >> 1) * 10 + j], acc);
            tile[e] = acc;
        }
        for (int kc : packed) {
            const int k = kc >> 4, c = kc & 15, pk = qp_full_slot_pack(k, c, NCK);
            const double *base = qp_full_slot_general(pk) ? tile.data() : v.data();
            const double got = base[qp_full_slot_read(pk) / 8];
            double want = v[k * 10 + (c < 10 ? c : 0)];
            if (c >= 10) {
                want = 0.0;
                for (int j = 0; j < 10; j++) want = std::fma(cd[(c - 10) * 10 + j], v[k * 10 + j], want);
            }
            CHECK(bits(got) == bits(want), "N = %d trial %d slot (%d, %d): %a, the chain per slot gives %a", N, trial, k, c, got, want);
        }
    }
    std::printf("N = %d: %d general-row slots, %d box slots\n", N, general, boxes);
}

int main()
{
    check_table(40);
    check_table(2);
    for (int N = 2; N <= 64; N++) {
        CHECK(qp_general_rows_inside(qp_lds(N, qp_lds_class(0, true)), N), "N = %d: the reach statement", N);
        for (int k = 0; k < N; k++)
            for (int row = 0; row < 2; row++) {
                const int pk = qp_full_slot_pack(k, 10 + row, 12);
                CHECK(qp_full_slot_read(pk) == 8 * (2 * k + row) && qp_full_slot_word(pk) == 8 * (k * 12 + 10 + row) && qp_full_slot_general(pk), "N = %d (%d, %d)", N, k, row);
            }
    }
    // beyond 68 stages the rows would leave the tile: the statement must say so
    CHECK(!qp_general_rows_inside(qp_lds(69, qp_lds_class(0, true)), 69), "2 N = 138 words do not fit the tile's 136");
    std::printf(fails ? "%d checks FAILED\n" : "all checks passed\n", fails);
    return fails ? 1 : 0;
}
