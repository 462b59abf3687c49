// qp_mrows.hpp -- where a double of M_k = A_k - B_k K_k lives in an instance's block of q_M (N x 512 bytes), described once: the factor
// sweep's stores (riccati_mfma.hpp), the vector and forward sweeps' loads (kernels_qp.hip: stream_rows) and the reach of their unclamped
// prefetch take their byte offsets from here.  Two layouts:
//   * stage-major, (N, 64) doubles with entry (row, col) of stage k at RIC_IDX: every kernel with a run-time horizon, every NF = 0
//     instantiation, the earlier form of the sweeps (stream_rows_v1) and the four-wave kernel;
//   * stage-PAIR-major, for the compiled-in horizon (NF > 0): pair q = k >> 1 is one row of 64 x 16 bytes, and lane (g, w) = (lane >> 3,
//     lane & 7) of the sweeps owns the 16 bytes { M_2q[g][w], M_2q+1[w][g] } of it -- the two values it takes in two consecutive steps of
//     EITHER sweep: the forward sweep wants M_k[g][w] at even k and M_k[w][g] at odd k; the vector sweep starts at k = N - 1 with its
//     "even" step on M_k[w][g], then M_k-1[g][w], so its step parity is the opposite of the stage parity exactly when N is even.  One
//     16-byte load per two stages then serves both.  An odd horizon has no such layout: the offset functions refuse it (-1).
// Nobody but the QP kernel that wrote a block reads it (the block is workspace: rewritten by every factorisation before it is read).
// Plain C++17 with no HIP header: tools/probes/check_qp_mrows.cpp builds it with g++ and walks it.
#pragma once

#ifdef __HIPCC__
#define QP_MROWS_FN __host__ __device__ constexpr
#else
#define QP_MROWS_FN constexpr
#endif

namespace ihm2 {

constexpr int QM_STAGE_BYTES = 512, QM_PAIR_BYTES = 2 * QM_STAGE_BYTES;

// stage-major: byte of entry (row, col) of stage k -- RIC_IDX (riccati_mfma.hpp) in bytes: rows r and r + 4 of a column are adjacent
QP_MROWS_FN int qm_stage_byte(int k, int row, int col) { return k * QM_STAGE_BYTES + (((((row & 3) * 8 + col) << 1) + (row >> 2)) << 3); }

QP_MROWS_FN bool qm_pair_horizon(int N) { return N > 0 && N % 2 == 0; }
// pair-major, writer: byte of entry (row, col) of stage k
QP_MROWS_FN int qm_pair_write(int N, int k, int row, int col)
{
    if (!qm_pair_horizon(N) || k < 0 || k >= N) return -1;
    return ((k >> 1) * 64 + ((k & 1) ? col * 8 + row : row * 8 + col)) * 16 + (k & 1) * 8;
}
// pair-major, reader: the 16 bytes of lane `lane` for the pair of stage k (the same in both sweeps) ...
QP_MROWS_FN int qm_pair_slot(int N, int k, int lane) { return qm_pair_horizon(N) ? ((k >> 1) * 64 + lane) * 16 : -1; }
// ... and the byte of the value the lane takes at stage k.  forward: step = k; backward: step = N - 1 - k.  A lane's even step takes the first
// element the sweep names (forward M[g][w], backward M[w][g]), its odd step the other: for an even N that is the half k & 1 in both.
QP_MROWS_FN int qm_pair_read(int N, int k, int lane, bool backward)
{
    if (!qm_pair_horizon(N) || k < 0 || k >= N) return -1;
    const int step = backward ? N - 1 - k : k;
    const int half = backward ? 1 - (step & 1) : (step & 1);
    return qm_pair_slot(N, k, lane) + half * 8;
}
// (row, col) of the value a sweep wants in lane (g, w) at a step of the given parity: what stream_rows' callers name
QP_MROWS_FN int qm_sweep_row(int lane, bool backward, bool odd_step) { return (backward != odd_step) ? (lane & 7) : (lane >> 3); }
QP_MROWS_FN int qm_sweep_col(int lane, bool backward, bool odd_step) { return (backward != odd_step) ? (lane >> 3) : (lane & 7); }

// The sweeps' prefetch runs UNCLAMPED: a pass is `ring` pairs (2 ring stages), the ring holds `ring` pairs, each refilled when its second
// stage has taken its value -- ceil(N / 2 ring) passes fetch ring (passes + 1) pair rows, of which N / 2 belong to the instance.  [lo, hi)
// in bytes from the start of the instance's block, over both directions.
struct QmReach { int lo, hi; };
QP_MROWS_FN int qm_pair_rows_fetched(int N, int ring) { return ((N + 2 * ring - 1) / (2 * ring) + 1) * ring; }
QP_MROWS_FN QmReach qm_pair_reach(int N, int ring)
{
    return {(N / 2 - qm_pair_rows_fetched(N, ring)) * QM_PAIR_BYTES, qm_pair_rows_fetched(N, ring) * QM_PAIR_BYTES};
}
// inside the allocation: q_M is padded by pad_rows stage rows in front of the first instance and behind the last
QP_MROWS_FN bool qm_pair_inside(int N, int ring, int pad_rows)
{
    const QmReach r = qm_pair_reach(N, ring);
    return qm_pair_horizon(N) && r.lo >= -pad_rows * QM_STAGE_BYTES && r.hi <= (N + pad_rows) * QM_STAGE_BYTES;
}

// the factor sweep's lane (g, j) holds rows g and g + 4 of column j and one running stage-major offset: at an even stage the pair-major
// byte IS the stage-major one, at an odd stage it differs by a constant of the lane
static_assert(qm_pair_write(40, 38, 3, 5) == qm_stage_byte(38, 3, 5) && qm_pair_write(40, 0, 0, 7) == qm_stage_byte(0, 0, 7), "even stages: same byte for rows 0..3");
QP_MROWS_FN int qm_pair_odd_delta(int N, int g, int j) { return qm_pair_write(N, 1, g, j) - qm_stage_byte(1, g, j); }
QP_MROWS_FN int qm_pair_row4_step(int N, bool odd) { return qm_pair_write(N, odd ? 1 : 0, 4, 0) - qm_pair_write(N, odd ? 1 : 0, 0, 0); }
static_assert(qm_pair_row4_step(40, false) == 512 && qm_pair_row4_step(40, true) == 64, "rows g and g + 4 of a column: 32 lanes or 4 lanes apart");

// The store schedule of the factor sweep (riccati_mfma.hpp, PLAIN, NF > 0): at stage k its lane (g, j) = (lane >> 4, lane & 15), j < 8, stores
// 8 bytes at qm_pair_write(N, k, g, j) and 8 bytes at qm_pair_write(N, k, g + 4, j) -- at an odd stage the second halves of the sweeps' slots
// j * 8 + g and j * 8 + g + 4, one stage later, at the even stage of the pair, the first halves of the slots g * 8 + j and (g + 4) * 8 + j.
// The two halves of a slot are therefore formed in DIFFERENT lanes of the factor sweep unless the slot lies on the diagonal: one 16-byte store
// per slot would take the odd stage's values across lanes (the 8 x 8 transpose the layout was made to avoid), not just one stage further.
QP_MROWS_FN int qm_factor_lane(int row, int col) { return (row & 3) * 16 + col; }                 // the lane that forms M_k[row][col] (in S[2] for row < 4, S[3] else)
QP_MROWS_FN int qm_pair_half_holder(int slot_lane, int half)                                      // half 0: the even stage's M[g][w], half 1: the odd stage's M[w][g]
{
    return half ? qm_factor_lane(slot_lane & 7, slot_lane >> 3) : qm_factor_lane(slot_lane >> 3, slot_lane & 7);
}
QP_MROWS_FN int qm_pair_slots_formed_in_one_lane()
{
    int n = 0;
    for (int lane = 0; lane < 64; lane++) n += qm_pair_half_holder(lane, 0) == qm_pair_half_holder(lane, 1);
    return n;
}
static_assert(qm_pair_slots_formed_in_one_lane() == 8, "only the diagonal slots have both halves in one lane of the factor sweep");

}  // namespace ihm2
