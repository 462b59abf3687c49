// qp_lds.hpp -- the LDS of one instance of the interior-point QP (kernels_qp.hip: qp_wave_body), described once: the arrays with their
// offsets and lengths in doubles, the total the launch asks for (qp_select.hpp: select_qp, select_steps), the integer offsets the factor sweep takes
// (riccati_mfma.hpp: RicLds; qp_lds_ric), and -- as checked statements -- how far the code that relies on an array's neighbours reaches.
// Plain C++17 with no HIP header: tools/probes/check_qp_lds.cpp builds it with g++ and walks every class over N = 2..64.
#pragma once

#include <cstddef>

#ifdef __HIPCC__
#define QP_LDS_FN __host__ __device__ constexpr
#else
#define QP_LDS_FN constexpr
#endif

namespace ihm2 {

// the transpose tile of the factor sweep, (8,17): rows padded to 17 against bank conflicts.  Outside the general sweep it is free: the
// straight-line stage parks its idle lanes' stores in it and the four-wave kernel takes its block reductions through it.
constexpr int QP_TILE_ROW = 17, QP_TILE_WORDS = 8 * QP_TILE_ROW;
// ring depth and LDS look-ahead of the sweeps' earlier form (kernels_qp.hip: stream_rows_v1), which the SQP loops keep
constexpr int QP_V1_RING = 8, QP_V1_DL = 4;
// the dynamic models' RK4 integrator in k_steps parks its base sensitivities at sm + lane, entry-major: this many words per lane
// (device_steps.hpp: s_count(1), asserted in kernels_qp.hip)
constexpr int QP_DYN_RK4_WORDS = 55;

// What the layout depends on besides N.  nck: constraint rows per stage held in LDS -- 8 x boxes, 2 u boxes, 2 general rows (+ 2 track
// rows (+ the lateral-acceleration row)).  hl / cl: the batch-shared stage Hessian / general rows are kept in LDS.
struct QpLdsClass { int nck; bool hc, ha, hl, cl; };
// from the template parameters of an instantiation; on the host PATH = alat_on ? 2 : path_on ? 1 : 0 and UNI = uniform_H && uniform_CD.
// UNI: H_0..H_{N-1} and [C D]_k do not depend on k; H is kept only where the budget of 40 KB per instance allows (no track rows).
QP_LDS_FN QpLdsClass qp_lds_class(int path, bool uni) { return {path == 2 ? 15 : path ? 14 : 12, path != 0, path == 2, uni && !path, uni}; }

struct QpArr {
    int off, len;
    QP_LDS_FN operator int() const { return off; }
    QP_LDS_FN int end() const { return off + len; }
};

struct QpLds {
    QpArr z;        // NS*10   QP iterate
    QpArr gt;       // NS*10   stationarity residual / modified gradient
    QpArr pi;       // NS*8    QP costates
    QpArr pv;       // NS*8    Riccati vector p_k, then dpi_k
    QpArr rb;       // N*8     dynamics residual
    QpArr gam;      // NS*NCK  barrier weights per constraint slot
    QpArr cf;       // NS*NCK  lam_l - lam_u, then gradient coefficients
    QpArr dz;       // NS*10   step
    QpArr kff;      // N*4     feed-forward terms (2 used per stage)
    QpArr Kl;       // N*16    K_k = Guu^-1 Gux
    QpArr Ginv;     // N*8     Guu^-1 as (Gi0, Gi1, Gi2, Gi1, 0, 0, 0, 0)
    QpArr Prb;      // N*8     P_{k+1} rb_k (same for predictor and corrector)
    QpArr tile;     // 8*17    transpose tile of the factor sweep
    QpArr hc;       // NS*2    d h_R / d psi, d h_L / d psi of the track rows (hc only)
    QpArr ha;       // NS*4    d a_lat / d (v_x, v_y, T, delta) of the lateral-acceleration row (ha only; zeros where the row is absent)
    QpArr Hl;       // 200     stage and terminal Hessian (hl only)
    QpArr CDl;      // 20      general rows (cl only)
    QpArr spv;      // 60      the (up to three) non-zeros of every row of the two Hessians (hl only) ...
    QpArr spc;      // 60 ints ... and their columns
    int total;
};
constexpr int QP_LDS_ARRAYS = 19;
QP_LDS_FN QpArr qp_lds_array(const QpLds &l, int i)      // in declaration order
{
    const QpArr a[QP_LDS_ARRAYS] = {l.z, l.gt, l.pi, l.pv, l.rb, l.gam, l.cf, l.dz, l.kff, l.Kl, l.Ginv, l.Prb, l.tile, l.hc, l.ha, l.Hl, l.CDl, l.spv, l.spc};
    return a[i];
}

// The length of every array, in doubles: the one place it is written.  (A function of its own, evaluated where it is asked for: the kernel forms
// its pointers as a chain by these lengths, and computing them all ahead -- or the pointers as sm + offset -- is the same arithmetic in another
// order, which moves the register allocation of every QP kernel.)
enum QpArrId { QP_Z, QP_GT, QP_PI, QP_PV, QP_RB, QP_GAM, QP_CF, QP_DZ, QP_KFF, QP_KL, QP_GINV, QP_PRB, QP_TILE, QP_HC, QP_HA, QP_HL, QP_CDL, QP_SPV, QP_SPC };
QP_LDS_FN int qp_lds_len(int id, int N, int NS, QpLdsClass c)
{
    switch (id) {
    case QP_Z: case QP_GT: case QP_DZ: return NS * 10;
    case QP_PI: case QP_PV: return NS * 8;
    case QP_GAM: case QP_CF: return NS * c.nck;
    case QP_RB: case QP_GINV: case QP_PRB: return N * 8;
    case QP_KFF: return N * 4;
    case QP_KL: return N * 16;
    case QP_TILE: return QP_TILE_WORDS;
    case QP_HC: return c.hc ? NS * 2 : 0;
    case QP_HA: return c.ha ? NS * 4 : 0;
    case QP_HL: return c.hl ? 200 : 0;
    case QP_CDL: return c.cl ? 20 : 0;
    case QP_SPV: return c.hl ? 60 : 0;
    default: return c.hl ? 30 : 0;      // QP_SPC: 60 ints
    }
}

QP_LDS_FN QpLds qp_lds(int N, QpLdsClass c)
{
    QpLds l = {};
    QpArr *const a[QP_LDS_ARRAYS] = {&l.z, &l.gt, &l.pi, &l.pv, &l.rb, &l.gam, &l.cf, &l.dz, &l.kff, &l.Kl, &l.Ginv, &l.Prb, &l.tile, &l.hc, &l.ha, &l.Hl, &l.CDl, &l.spv, &l.spc};
    for (int id = 0; id < QP_LDS_ARRAYS; id++) {       // the members in declaration order = the order of QpArrId
        *a[id] = {l.total, qp_lds_len(id, N, N + 1, c)};
        l.total += a[id]->len;
    }
    return l;
}

// The offsets the factor sweep takes (riccati_mfma.hpp: RicLds), in the closed forms the kernels have always handed it: the stage arrays in
// front as multiples of NS = N + 1, the rest as a chain from gam.  The same numbers as the layout's -- asserted here for N = 40 and N = 2 and
// walked for N = 2..64 by check_qp_lds.cpp -- but the QP kernels' register allocation follows the SHAPE of this integer arithmetic: formed as
// the layout's running sums, the offsets moved between 300 and 6000 instructions in every kernel with a run-time horizon.  (ha supposes hc:
// the a_lat row comes with the track rows.)
struct QpRic { int gt, pv, gam, dz, kff, Kl, Ginv, Prb, tile, hc, ha; };
QP_LDS_FN QpRic qp_lds_ric(int N, int NS, int nck)
{
    QpRic L = {};
    L.gt = NS * 10; L.pv = NS * 28; L.gam = NS * 36 + N * 8; L.dz = L.gam + 2 * NS * nck; L.kff = L.dz + NS * 10; L.Kl = L.kff + N * 4;
    L.Ginv = L.Kl + N * 16; L.Prb = L.Ginv + N * 8; L.tile = L.Prb + N * 8; L.hc = L.tile + QP_TILE_WORDS; L.ha = L.hc + NS * 2;
    return L;
}
QP_LDS_FN bool qp_lds_ric_agrees(int N, QpLdsClass c)
{
    const QpLds l = qp_lds(N, c);
    const QpRic o = qp_lds_ric(N, N + 1, c.nck);
    return o.gt == l.gt && o.pv == l.pv && o.gam == l.gam && o.dz == l.dz && o.kff == l.kff && o.Kl == l.Kl && o.Ginv == l.Ginv && o.Prb == l.Prb &&
           o.tile == l.tile && o.hc == l.hc && (!c.hc || o.ha == l.ha);
}
QP_LDS_FN bool qp_lds_ric_agrees(int N)
{
    return qp_lds_ric_agrees(N, qp_lds_class(0, false)) && qp_lds_ric_agrees(N, qp_lds_class(0, true)) && qp_lds_ric_agrees(N, qp_lds_class(1, false)) &&
           qp_lds_ric_agrees(N, qp_lds_class(1, true)) && qp_lds_ric_agrees(N, qp_lds_class(2, true));
}
static_assert(qp_lds_ric_agrees(40) && qp_lds_ric_agrees(2), "the factor sweep's offsets are not the layout's");

// ---- who relies on an array's neighbours, and how far: [lo, hi) in doubles from the start of the block's LDS ----
struct QpReach { int lo, hi; };
QP_LDS_FN bool qp_inside(QpReach r, int lo, int hi) { return lo <= r.lo && r.lo <= r.hi && r.hi <= hi; }

// The vector and forward sweeps fetch their LDS operands UNCLAMPED, dl stages ahead, in passes of 2 d stages (kernels_qp.hip:
// stream_rows): dl + 2 d ceil(N / 2 d) fetches, even and odd steps in turn; the values fetched for stages outside [0, N) are never used.
QP_LDS_FN int qp_sweep_fetches(int N, int d, int dl) { return dl + (N + 2 * d - 1) / (2 * d) * 2 * d; }
// lean form: running pointers.  Vector sweep: Prb and pv from the rows N-1 (even steps) and N-2 (odd steps) downwards, 16 words per two
// stages; forward sweep: dz from the rows 1 and 2 upwards, 20 words per two stages.  (Idle lanes read the zero word dz[0].)
QP_LDS_FN QpReach qp_reach_lean_vector(const QpLds &l, int N, int d, int dl)
{
    return {l.pv + (N - 2) * 8 - 16 * (qp_sweep_fetches(N, d, dl) / 2 - 1), l.Prb + N * 8};
}
QP_LDS_FN QpReach qp_reach_lean_forward(const QpLds &l, int N, int d, int dl)
{
    return {l.dz, l.dz + 20 + 20 * (qp_sweep_fetches(N, d, dl) / 2 - 1) + 8};
}
// earlier form: indexed by the stage.  Vector sweep: the rows k of Prb and pv for k = N-1 down to N - qp_sweep_fetches; forward sweep:
// the rows k + 1 of dz for k = 0 up to qp_sweep_fetches - 1.
QP_LDS_FN QpReach qp_reach_v1_vector(const QpLds &l, int N)
{
    return {l.pv + (N - qp_sweep_fetches(N, QP_V1_RING, QP_V1_DL)) * 8, l.Prb + N * 8};
}
QP_LDS_FN QpReach qp_reach_v1_forward(const QpLds &l, int N)
{
    return {l.dz, l.dz + qp_sweep_fetches(N, QP_V1_RING, QP_V1_DL) * 10 + 8};
}
// The straight-line factor stage (riccati_mfma.hpp: PLAIN).  Lanes that own no entry of an output array store to tile + lane, at most
// 4 words further (the second register of a pair) ...
QP_LDS_FN QpReach qp_reach_plain_parking(const QpLds &l) { return {l.tile, l.tile + 63 + 4 + 1}; }
// ... and the next stage's C operand is read unconditionally: after stage 0 the rows "k = -1" of gt and gam, i.e. the words in front of
// them (gt comes first); upwards the lane groups 2, 3 read the words 10, 11 of a row of 10 -- the next row's, at most row N-1's.
QP_LDS_FN QpReach qp_reach_plain_operand(const QpLds &l, int N, int nck) { return {l.gt - 10, l.gam + N * nck}; }
// ... and what it STORES to LDS: p_N into the terminal row of pv; P_{k+1} rb_k, Guu^-1, kff_k, K_k into their own rows 0 .. N-1; c_k into
// the rows 1 .. N of dz (+ 4: the second register of a pair); everything else into the parking words of the tile.  The lowest of them
// besides pv's row is dz + 10, the highest the end of the tile.
QP_LDS_FN QpReach qp_reach_plain_stores(const QpLds &l) { return {l.dz + 10, l.tile.end()}; }
QP_LDS_FN QpReach qp_reach_plain_store_pv(const QpLds &l, int N) { return {l.pv + N * 8, l.pv + N * 8 + 8}; }
// The full slot form (kernels_qp.hip: qp_wave_body, FULL) zeroes gam and cf ONCE per solve, where the general form zeroes them in every
// coefficient pass.  The writers of the two arrays, walked one by one:
//   * the slot loops (multipliers_to_cf, slot_coeffs): slot (k, c) stores to the word k nck + c of cf in every pass, and of gam in the
//     predictor's pass -- in a full table every slot of every lane, unconditionally, so an owned word is rewritten before each of its readers
//     (the exact residual, add_coeffs, the factor sweep) as it is after the zeroing pass of the general form; the words no slot owns
//     (stage 0's state boxes, stage N's input and general rows, unbounded states) are written by nobody;
//   * the factor sweep: its stores are qp_reach_plain_stores and qp_reach_plain_store_pv, both outside [gam, cf.end); its "k = -1" operand
//     (qp_reach_plain_operand) is a read;
//   * the vector and forward sweeps store to pv and dz inside [0, N) only (their unclamped accesses are prefetches: reads);
//   * the four-wave kernel parks its slot sums in gam: it has no full form.
// So a word of gam or cf is either rewritten by its one owning slot in every pass or never written after the zeroing at the top.
QP_LDS_FN bool qp_full_zeroes_kept(const QpLds &l, int N)
{
    const QpReach s = qp_reach_plain_stores(l), p = qp_reach_plain_store_pv(l, N);
    return s.lo >= l.cf.end() && qp_inside(s, l.cf.end(), l.total) && qp_inside(p, 0, l.gam) && l.cf == l.gam.end();
}
// The full slot form evaluates the general rows [C D] v_k once per phase (kernels_qp.hip: general_rows): element e = 2 k + row of the
// stages k < N goes to tile[e], and a general-row slot reads its word back from there.  The tile is shared with the straight-line factor
// stage, which parks its idle lanes' stores in it (qp_reach_plain_parking), so a word of it holds nothing across a factor sweep: the pass
// rewrites ALL the words a slot can read -- [tile, tile + 2 N) -- behind the sweep and before the first read of each phase, and no slot
// reads a word outside them (qp_full_slot_pack below: the offsets 8 (2 k + row), k < N).  Parked words at 2 N and above are read by nobody.
QP_LDS_FN QpReach qp_reach_general_rows(const QpLds &l, int N) { return {l.tile, l.tile + 2 * N}; }
QP_LDS_FN bool qp_general_rows_inside(const QpLds &l, int N) { return qp_inside(qp_reach_general_rows(l, N), l.tile, l.tile.end()); }
static_assert(qp_general_rows_inside(qp_lds(40, qp_lds_class(0, true)), 40) && qp_general_rows_inside(qp_lds(2, qp_lds_class(0, true)), 2),
              "the general rows of a phase leave the transpose tile");
// What the full slot form keeps of the slot (k, c) in its one register: bits 0..15 the byte offset 8 (k nck + c) of its word in cf and
// gam; bits 16..29 the byte offset of the word a phase reads for R_c . v -- of a box row (c < 10) its word 8 (k 10 + c) in the stage-major
// vector v[NS][10], of a general row its word 8 (2 k + c - 10) in the tile; bit 31 (the sign) a general row, bit 30 which of the two.
QP_LDS_FN int qp_full_slot_pack(int k, int c, int nck)
{
    return ((k * nck + c) * 8) | ((c < 10 ? k * 10 + c : 2 * k + (c - 10)) << 19) | ((c >= 10) ? (int)(0x80000000u | ((unsigned)(c - 10) << 30)) : 0);
}
QP_LDS_FN bool qp_full_slot_general(int pk) { return pk < 0; }
QP_LDS_FN int qp_full_slot_read(int pk) { return (pk >> 16) & 0x3fff; }      // the byte offset of the bits 16..29
QP_LDS_FN int qp_full_slot_word(int pk) { return pk & 0xffff; }             // the byte offset of the bits 0..15
// the four-wave kernel's block reductions: one word per wave, in the tile
QP_LDS_FN QpReach qp_reach_block_reduce(const QpLds &l, int nw) { return {l.tile, l.tile + nw}; }

// every reach of the sweeps in the given form (lean with ring depth d and look-ahead dl, else the earlier form) inside the block
QP_LDS_FN bool qp_sweeps_inside(const QpLds &l, int N, bool lean, int d, int dl)
{
    return lean ? qp_inside(qp_reach_lean_vector(l, N, d, dl), 0, l.total) && qp_inside(qp_reach_lean_forward(l, N, d, dl), 0, l.total)
                : qp_inside(qp_reach_v1_vector(l, N), 0, l.total) && qp_inside(qp_reach_v1_forward(l, N), 0, l.total);
}
// the reaches that do not depend on the sweeps' form: parking and reductions inside the tile, the operand reads inside the block
QP_LDS_FN bool qp_factor_inside(const QpLds &l, int N, int nck)
{
    return qp_inside(qp_reach_plain_parking(l), l.tile, l.tile.end()) && qp_inside(qp_reach_block_reduce(l, 4), l.tile, l.tile.end()) &&
           qp_inside(qp_reach_plain_operand(l, N, nck), 0, l.total);
}

// ---- the x0-sensitivity body (sens_body.hpp): k_sens' whole LDS, and the persistent loop's guest with SENS = 1 ----
constexpr int SENS_ROWS = 15;       // rows per stage: 8 state boxes, 2 input boxes, 2 general rows, 2 track rows, the lateral-acceleration row
// LDS of the factorisation (doubles): the arrays w .. Q that sens_body and k_adj carve out in front of their own; sens_factor_body.hpp fills them
QP_LDS_FN size_t sens_factor_lds_doubles(size_t N) { return (N + 1) * (SENS_ROWS + 6) + N * 16 + 64 + 64 + 16 + 100 + 64 + 16 + 84; }
// LDS of one instance (doubles): the factorisation's arrays and the forward sweep's dX_k (64), dU_k (16) behind them (sens_body's carve-up)
QP_LDS_FN size_t sens_lds_doubles(size_t N) { return sens_factor_lds_doubles(N) + 64 + 16; }
static_assert(sens_lds_doubles(40) == 1989 && sens_lds_doubles(1) == 546, "k_sens: launch LDS at N = 40 and N = 1");

// ---- k_steps: the QP's LDS and its guests ----
// qp: the QP's own; sens: sens_body's, from offset 0 (0 without SENS); dyn_rk4: the dynamic models' RK4 integrator, QP_DYN_RK4_WORDS per
// lane from offset 0 (0 otherwise).  The launch is sized for the QP and the sensitivities; it is not enlarged for the integrator: a QP
// smaller than that (short horizons) is launched per step instead.
struct StepsLds {
    int qp, sens, dyn_rk4;
    QP_LDS_FN int total() const { return qp > sens ? qp : sens; }
    QP_LDS_FN bool guests_fit() const { return dyn_rk4 <= total(); }
};
QP_LDS_FN StepsLds steps_lds_doubles(int qp_total, int sens_doubles, bool dyn_rk4) { return {qp_total, sens_doubles, dyn_rk4 ? QP_DYN_RK4_WORDS * 64 : 0}; }

}  // namespace ihm2
