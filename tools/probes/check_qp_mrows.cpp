// The stage-pair-major layout of M_k (ihm2_amd/csrc/qp_mrows.hpp) walked on the CPU, as a program of its own: for every even N in 2..64
//   * the writer's bytes: every (k, row, col) lands on its own 8 bytes of the instance's block, the block is covered exactly once, and what
//     the factor sweep's lane (g, j) forms from its running stage-major offset (riccati_mfma.hpp: gofs, + the lane's constant at odd stages,
//     + the row-4 step) are those bytes;
//   * the factor sweep's store schedule replayed (two 8-byte stores per lane and stage, k = N - 1 .. 0): every byte of the block written exactly
//     once by the end of the sweep, none outside it, each half by the lane qm_pair_half_holder names -- and only the 8 diagonal slots have both
//     halves in one lane (why a 16-byte store per slot is not "hold the odd stage's values for one stage");
//   * the readers: lane (g, w) of the forward sweep gets M_k[g][w] at even k and M_k[w][g] at odd k; the backward sweep gets M_k[w][g] on its
//     even steps and M_k[g][w] on its odd steps (step = N - 1 - k); both from the lane's one 16-byte slot of the pair;
//   * a replay of stream_rows' paired fetch sequence (prologue of `ring` pair rows, then one refill per pair of every pass) touches exactly
//     qm_pair_reach, and that lies inside q_M's padding of QM_PAD stage rows for the first and the last instance of a batch;
// and every odd N is refused by every offset function.  N = 40 with the kernels' ring depth is the shipped case and is printed.
// Build: g++ -std=c++17 -I ihm2_amd/csrc tools/probes/check_qp_mrows.cpp   (SWEEP_RING, QM_PAD as in the kernels; also with -fsanitize=address,undefined)
#include <algorithm>
#include <cstdio>
#include <vector>

#include "qp_mrows.hpp"

using namespace ihm2;

#ifndef SWEEP_RING
#define SWEEP_RING 4
#endif
#ifndef QM_PAD
#define QM_PAD 24
#endif

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

int main()
{
    for (int N = 2; N <= 64; N += 2) {
        // ---- writer: value id (k, row, col) -> its byte; the block as an array of doubles holding ids ----
        std::vector<int> block(N * 64, -1);
        for (int k = 0; k < N; k++)
            for (int row = 0; row < 8; row++)
                for (int col = 0; col < 8; col++) {
                    const int byte = qm_pair_write(N, k, row, col);
                    CHECK(byte >= 0 && byte % 8 == 0 && byte + 8 <= N * QM_STAGE_BYTES, "N %d k %d (%d, %d): byte %d", N, k, row, col, byte);
                    if (byte < 0 || byte % 8 || byte + 8 > N * QM_STAGE_BYTES) continue;
                    CHECK(block[byte / 8] == -1, "N %d k %d (%d, %d): byte %d written twice", N, k, row, col, byte);
                    block[byte / 8] = (k * 8 + row) * 8 + col;
                }
        CHECK(std::count(block.begin(), block.end(), -1) == 0, "N %d: words nobody writes", N);
        // the factor sweep's arithmetic: lane (g, j), g = 0..3, j = 0..7, running offset = the stage-major byte of (k, g, j)
        for (int k = 0; k < N; k++)
            for (int g = 0; g < 4; g++)
                for (int j = 0; j < 8; j++) {
                    const bool odd = (k & 1) != 0;
                    const int at = qm_stage_byte(k, g, j) + (odd ? qm_pair_odd_delta(N, g, j) : 0);
                    CHECK(at == qm_pair_write(N, k, g, j) && at + qm_pair_row4_step(N, odd) == qm_pair_write(N, k, g + 4, j), "N %d k %d lane (%d, %d)", N, k, g, j);
                }
        // ---- the store schedule replayed: the sweep runs k = N - 1 .. 0, every lane (g, j), j < 8, stores its two 8-byte halves per stage; every
        // byte of the block is written exactly once, all of it by the end of the sweep (the caller's barrier stands behind it), nothing outside;
        // and the lane that stores a half is the lane qm_pair_half_holder names for the slot the half belongs to ----
        {
            std::vector<int> written(N * QM_STAGE_BYTES, 0);
            int outside = 0, wrong_holder = 0, whole = 0;
            for (int k = N - 1; k >= 0; k--)
                for (int lane = 0; lane < 64; lane++) {
                    const int g = lane >> 4, j = lane & 15;
                    if (j >= 8) continue;
                    const bool odd = (k & 1) != 0;
                    const int at0 = qm_stage_byte(k, g, j) + (odd ? qm_pair_odd_delta(N, g, j) : 0), at[2] = {at0, at0 + qm_pair_row4_step(N, odd)};
                    for (int h = 0; h < 2; h++) {
                        if (at[h] < 0 || at[h] + 8 > N * QM_STAGE_BYTES) { outside++; continue; }
                        for (int b = 0; b < 8; b++) written[at[h] + b]++;
                        const int slot = (at[h] % QM_PAIR_BYTES) / 16, half = (at[h] % 16) / 8;
                        CHECK(half == (k & 1) && at[h] / QM_PAIR_BYTES == (k >> 1), "N %d k %d lane %d: half %d of pair %d", N, k, lane, half, at[h] / QM_PAIR_BYTES);
                        if (qm_pair_half_holder(slot, half) != lane) wrong_holder++;
                    }
                }
            CHECK(outside == 0, "N %d: %d stores outside the block", N, outside);
            CHECK(std::count(written.begin(), written.end(), 1) == N * QM_STAGE_BYTES, "N %d: a byte written twice or not at all", N);
            CHECK(wrong_holder == 0, "N %d: %d halves stored by another lane than qm_pair_half_holder names", N, wrong_holder);
            for (int slot = 0; slot < 64; slot++) whole += qm_pair_half_holder(slot, 0) == qm_pair_half_holder(slot, 1);
            CHECK(whole == 8 && whole == qm_pair_slots_formed_in_one_lane(), "slots with both halves in one lane: %d", whole);
            if (N == 40) std::printf("N 40 writer: %d bytes written once, %d of 64 slots have both halves in one lane of the factor sweep\n", N * QM_STAGE_BYTES, whole);
        }
        // ---- readers ----
        for (int k = 0; k < N; k++)
            for (int lane = 0; lane < 64; lane++) {
                const int g = lane >> 3, w = lane & 7;
                for (int backward = 0; backward < 2; backward++) {
                    const int step = backward ? N - 1 - k : k;
                    const bool odd_step = (step & 1) != 0;
                    const int byte = qm_pair_read(N, k, lane, backward != 0);
                    CHECK(byte >= qm_pair_slot(N, k, lane) && byte + 8 <= qm_pair_slot(N, k, lane) + 16, "N %d k %d lane %d: outside the lane's slot", N, k, lane);
                    // what the sweep's caller names: forward (g, w) then (w, g); backward (w, g) then (g, w)
                    const int row = backward ? (odd_step ? g : w) : (odd_step ? w : g), col = backward ? (odd_step ? w : g) : (odd_step ? g : w);
                    CHECK(row == qm_sweep_row(lane, backward != 0, odd_step) && col == qm_sweep_col(lane, backward != 0, odd_step), "the sweeps' element, lane %d", lane);
                    CHECK(byte >= 0 && block[byte / 8] == (k * 8 + row) * 8 + col, "N %d k %d lane %d %s: reads id %d, wants M[%d][%d]", N, k, lane,
                          backward ? "backward" : "forward", byte >= 0 ? block[byte / 8] : -1, row, col);
                    // by stage parity: forward even k -> M[g][w], odd k -> M[w][g]
                    if (!backward) CHECK((k & 1) ? (row == w && col == g) : (row == g && col == w), "forward parity");
                }
            }
        // ---- the unclamped prefetch: replay of the paired stream_rows, pair rows relative to the instance ----
        for (int ring = 2; ring <= 8; ring += 2) {
            int lo = 1 << 30, hi = -(1 << 30), loads = 0;
            for (int dir = -1; dir <= 1; dir += 2) {
                auto load_pair = [&](int pstep) {
                    const int prow = dir < 0 ? N / 2 - 1 - pstep : pstep;
                    lo = std::min(lo, prow * QM_PAIR_BYTES); hi = std::max(hi, (prow + 1) * QM_PAIR_BYTES);
                    loads++;
                };
                for (int p = 0; p < ring; p++) load_pair(p);
                for (int s0 = 0; s0 < N; s0 += 2 * ring)
                    for (int p = 0; p < ring; p++) load_pair(s0 / 2 + p + ring);
            }
            const QmReach r = qm_pair_reach(N, ring);
            CHECK(r.lo == lo && r.hi == hi && loads == 2 * qm_pair_rows_fetched(N, ring), "N %d ring %d: reach [%d, %d) against the replay's [%d, %d)", N, ring, r.lo, r.hi, lo, hi);
            const bool inside = lo >= -QM_PAD * QM_STAGE_BYTES && hi <= (N + QM_PAD) * QM_STAGE_BYTES;
            CHECK(qm_pair_inside(N, ring, QM_PAD) == inside, "N %d ring %d: qm_pair_inside", N, ring);
            if (ring == SWEEP_RING) CHECK(inside, "N %d: the kernels' ring of %d pairs leaves the padding: [%d, %d)", N, ring, lo, hi);
            if (N == 40 && ring == SWEEP_RING) std::printf("N 40 ring %d: fetches [%d, %d) of a block of %d bytes, padding %d\n", ring, lo, hi, N * QM_STAGE_BYTES, QM_PAD * QM_STAGE_BYTES);
        }
    }
    // ---- odd horizons are refused ----
    for (int N = 1; N <= 63; N += 2) {
        CHECK(!qm_pair_horizon(N) && qm_pair_write(N, 0, 0, 0) == -1 && qm_pair_read(N, 0, 0, false) == -1 && qm_pair_read(N, 0, 0, true) == -1 &&
              qm_pair_slot(N, 0, 0) == -1 && !qm_pair_inside(N, SWEEP_RING, QM_PAD), "odd N %d accepted", N);
    }
    CHECK(qm_pair_write(40, 40, 0, 0) == -1 && qm_pair_write(40, -1, 0, 0) == -1 && qm_pair_read(40, 40, 0, false) == -1, "stages outside [0, N) accepted");
    std::printf(fails ? "%d checks FAILED\n" : "all checks passed\n", fails);
    return fails ? 1 : 0;
}
