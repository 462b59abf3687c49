// The predicate that lets a handle take the QP kernels' full slot form (ihm2_amd/csrc/qp_tables.hpp: slot_table_full, slot_bounds_full
// on the slot images of table_images) evaluated on the CPU, through the functions api.hip calls: the reference's rows (state boxes on n, v_x, T, delta of the stages
// 1..N-1, on n, v_x, v_y, r of stage N, input boxes and the two rate rows on the stages 0..N-1) laid out for the all-hard
// instantiations of the catalogue.  One line per case: name full(0/1) per_lane total; then "all checks passed" if the table of every
// full case is what the kernel takes unasked.  No arguments.
// Build: g++ -std=c++17 -fsanitize=address,undefined -I ihm2_amd/csrc tools/probes/check_full_table.cpp
#include <cstdio>
#include <string>

#include "qp_catalogue.hpp"
#include "qp_tables.hpp"

using namespace ihm2;

static const int NSLOT_FULL = full_form_nslot();        // the NSLOT of the catalogue's full-form pair, as api.hip takes it
static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

struct Arrays {
    int N;
    std::vector<double> lbx, ubx, lbu, ubu, lg, ug;
};

// the reference's bounds at the horizon N; absent sides as the callers write them (+-1e20)
static Arrays reference_rows(int N)
{
    const int NS = N + 1;
    Arrays a{N, std::vector<double>(NS * 8, -1e20), std::vector<double>(NS * 8, 1e20), std::vector<double>(N * 2), std::vector<double>(N * 2),
             std::vector<double>(N * 2), std::vector<double>(N * 2)};
    const double lo[8] = {-50.0, -2.0, -0.9, 0.0, -4.0, -4.0, -500.0, -0.5}, hi[8] = {1e4, 2.0, 0.9, 31.0, 4.0, 4.0, 500.0, 0.5};
    const int stage[4] = {1, 3, 6, 7}, terminal[4] = {1, 3, 4, 5};
    for (int k = 1; k <= N; k++)
        for (int q = 0; q < 4; q++) {
            const int i = (k < N) ? stage[q] : terminal[q];
            a.lbx[k * 8 + i] = lo[i]; a.ubx[k * 8 + i] = hi[i];
        }
    for (int k = 0; k < N; k++) {
        a.lbu[k * 2] = -500.0; a.ubu[k * 2] = 500.0; a.lbu[k * 2 + 1] = -0.5; a.ubu[k * 2 + 1] = 0.5;
        a.lg[k * 2] = -5.0; a.ug[k * 2] = 5.0; a.lg[k * 2 + 1] = -0.02; a.ug[k * 2 + 1] = 0.02;
    }
    return a;
}

static ConstraintRows rows_of(const Arrays &a)
{
    ConstraintRows r(a.N + 1);
    r.set_box_rows(a.lbx.data(), a.ubx.data(), a.lbu.data(), a.ubu.data(), a.lg.data(), a.ug.data());
    r.set_track_rows(false, nullptr, nullptr);
    return r;
}

static SlotTable table_of(const ConstraintRows &r, int path = 0) { return lay_out_slots(r, slot_limits(path)); }

// what the kernel's full form takes unasked, stated once more from the table
static void check_taken_unasked(const SlotTable &t)
{
    CHECK(t.fit && t.nsoft == 0 && t.per_lane == NSLOT_FULL && t.entries() == (size_t)64 * NSLOT_FULL);
    std::vector<int> seen;
    for (size_t e = 0; e < t.entries(); e++) {
        const int k = t.kc[e] >> 4, c = t.kc[e] & 15;
        CHECK(t.kc[e] >= 0 && c < 12 && k >= 0);
        CHECK(std::fabs(t.lb[e]) < 1e20 && std::fabs(t.ub[e]) < 1e20 && t.Zw[e] < 0.0);
        for (int s : seen) CHECK(s != t.kc[e]);      // one slot per row: a slot's word of cf and gam is its own
        seen.push_back(t.kc[e]);
    }
}

static void report(const char *name, bool full, const SlotTable &t) { std::printf("%s %d %d %d\n", name, full ? 1 : 0, t.per_lane, t.total); }

int main()
{
    for (int N : {40, 8, 39, 41}) {
        const SlotTable t = table_of(rows_of(reference_rows(N)));
        const bool full = slot_table_full(t, NSLOT_FULL);
        report(("ref_N" + std::to_string(N)).c_str(), full, t);
        if (full) check_taken_unasked(t);
    }
    {       // one upper state bound infinite (stage 17, v_x), written as the setter's absent side and as a real infinity
        for (const double absent : {1e20, (double)INFINITY}) {
            Arrays a = reference_rows(40);
            a.ubx[17 * 8 + 3] = absent;
            const SlotTable t = table_of(rows_of(a));
            report(absent == 1e20 ? "one_upper_1e20" : "one_upper_inf", slot_table_full(t, NSLOT_FULL), t);
        }
    }
    {       // per-instance bounds: all finite -> full; one side of one instance infinite -> not full
        const int B = 3, N = 40, NS = N + 1;
        const Arrays a = reference_rows(N);
        const SlotTable t = table_of(rows_of(a));
        for (const bool broken : {false, true}) {
            std::vector<double> il((size_t)B * NS * 12), iu((size_t)B * NS * 12);
            for (int b = 0; b < B; b++) {
                Arrays ab = a;
                for (double &v : ab.ubu) v *= 1.0 - 0.1 * b;
                if (broken && b == 1) ab.lbx[23 * 8 + 6] = -INFINITY;
                box_rows(N, ab.lbx.data(), ab.ubx.data(), ab.lbu.data(), ab.ubu.data(), ab.lg.data(), ab.ug.data(), &il[(size_t)b * NS * 12], &iu[(size_t)b * NS * 12], 12);
            }
            const TableImages m = table_images(t, rows_of(a), B, il.data(), iu.data(), nullptr, nullptr, nullptr, nullptr);
            report(broken ? "instance_one_inf" : "instance_all_finite", slot_table_full(t, NSLOT_FULL) && slot_bounds_full(t, B, m.slot_lo, m.slot_up), t);
            // the predicate reads the bounds halves only, `entries` apart from the penalties: an all-hard table's Zw = -1 and zw = 0 are
            // finite, so an infinity planted in a penalty half must not change the answer, and one planted in a bounds half must
            TableImages p = m;
            p.slot_lo[(size_t)2 * 2 * t.entries() + t.entries() + 3] = INFINITY;
            CHECK(slot_bounds_full(t, B, p.slot_lo, p.slot_up) == !broken);
            p = m;
            p.slot_up[(size_t)2 * 2 * t.entries() + t.entries() - 1] = INFINITY;
            CHECK(!slot_bounds_full(t, B, p.slot_lo, p.slot_up));
        }
        {       // B = 1, nothing per instance: the shared table itself
            const TableImages m = table_images(t, rows_of(a), 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
            CHECK(m.entries == t.entries() && m.slot_lo.size() == 2 * t.entries() && slot_bounds_full(t, 1, m.slot_lo, m.slot_up));
            CHECK(std::equal(t.lb.begin(), t.lb.end(), m.slot_lo.begin()) && std::equal(t.zw.begin(), t.zw.end(), m.slot_lo.begin() + t.entries()));
            CHECK(std::equal(t.ub.begin(), t.ub.end(), m.slot_up.begin()) && std::equal(t.Zw.begin(), t.Zw.end(), m.slot_up.begin() + t.entries()));
        }
        // arrays of another shape than the table's are no evidence
        CHECK(!slot_bounds_full(t, B, std::vector<double>(5), std::vector<double>(5)));
        CHECK(!slot_bounds_full(t, B, std::vector<double>(B * t.entries(), 0.0), std::vector<double>(B * t.entries(), 0.0)));
    }
    {       // a soft table: the torque rate row's upper side soft on every stage
        ConstraintRows r = rows_of(reference_rows(40));
        for (int k = 0; k < 40; k++) { r.sz[k * NLAM + NC + 10] = 10.0; r.sZ[k * NLAM + NC + 10] = 1.0; }
        const SlotTable t = table_of(r);
        CHECK(t.fit && t.nsoft > 0);
        report("soft", slot_table_full(t, NSLOT_FULL), t);
    }
    {       // track rows: another class of instantiation, and rows 12, 13 in the table
        ConstraintRows r = rows_of(reference_rows(40));
        const double lh[2] = {-1e3, -1e3}, uh[2] = {0.0, 0.0};
        r.set_track_rows(true, lh, uh);
        const SlotTable t = table_of(r, 1);
        report("track_rows", slot_table_full(t, NSLOT_FULL), t);
    }
    {       // nothing laid out yet
        const SlotTable t;
        report("no_table", slot_table_full(t, NSLOT_FULL), t);
    }
    if (fails) return 1;
    std::printf("all checks passed\n");
    return 0;
}
