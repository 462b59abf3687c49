// The LDS layout of the interior-point QP (ihm2_amd/csrc/qp_lds.hpp) walked on the CPU: N = 2..64 (ihm2mpc_create refuses N = 1), every
// (PATH, UNI) class the catalogue of kernels_qp.hip instantiates.
//   * the arrays are disjoint, in declaration order, and sum to the total;
//   * the total and the factor sweep's integer offsets equal the closed forms api.hip and kernels_qp.hip held before the layout was
//     written down (copied here as the independent statement);
//   * the sweeps' reaches equal what a replay of stream_rows' fetch sequence touches, and every consumer's reach is inside the block --
//     except exactly the sweeps' earlier form at N = 2 and N = 3, whose reach is printed (qp_select.hpp: select_steps refuses those).
// Build: g++ -std=c++17 -I ihm2_amd/csrc tools/probes/check_qp_lds.cpp   (SWEEP_RING as in kernels_qp.hip; also with -fsanitize=address,undefined)
#include <algorithm>
#include <cstdio>

#include "qp_lds.hpp"

using namespace ihm2;

#ifndef SWEEP_RING
#define SWEEP_RING 4
#endif
#define SWEEP_DL ((SWEEP_RING >= 8) ? 4 : 2)

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// the fetches of stream_rows<DIR, D, DL>: pre(k', odd) for the prologue's DL stages, then one per stage of every pass of 2 D stages
template <typename F>
static void replay(int dir, int N, int D, int DL, F pre)
{
    for (int d = 0; d < DL; d++) pre(dir < 0 ? N - 1 - d : d, (d & 1) != 0);
    for (int s0 = 0; s0 < N; s0 += 2 * D)
        for (int s = s0; s < s0 + 2 * D; s++) {
            const int k = dir < 0 ? N - 1 - s : s;
            pre(dir < 0 ? k - DL : k + DL, ((s - s0) & 1) != 0);
        }
}
struct Hull {
    int lo = 1 << 30, hi = -(1 << 30);
    void word(int a) { lo = std::min(lo, a); hi = std::max(hi, a + 1); }
    bool is(QpReach r) const { return lo == r.lo && hi == r.hi; }
};

int main()
{
    const int classes[5][2] = {{0, 0}, {0, 1}, {1, 0}, {1, 1}, {2, 1}};
    for (const auto &pc : classes)
        for (int N = 2; N <= 64; N++) {
            const int path = pc[0], uni = pc[1], NS = N + 1;
            const QpLdsClass c = qp_lds_class(path, uni != 0);
            const QpLds l = qp_lds(N, c);
            // ---- arrays ----
            int p = 0;
            for (int i = 0; i < QP_LDS_ARRAYS; i++) {
                const QpArr a = qp_lds_array(l, i);
                CHECK(a.off == p && a.len >= 0, "array %d of path %d uni %d N %d", i, path, uni, N);
                p += a.len;
            }
            CHECK(p == l.total, "sum %d total %d", p, l.total);
            // ---- the closed forms held before (the launch's LDS bytes, qp_select.hpp: select_qp; kernels_qp.hip: the RicLds block) ----
            const int nck = path ? (path == 2 ? 15 : 14) : 12;
            const int total = NS * (10 + 10 + 8 + 8 + 2 * nck + 10 + (path ? (path == 2 ? 6 : 2) : 0)) + N * (8 + 4 + 16 + 8 + 8) + 136 + (uni ? 20 + (path ? 0 : 200 + 90) : 0);
            CHECK(l.total == total && c.nck == nck, "path %d uni %d N %d: %d against %d", path, uni, N, l.total, total);
            const int gam = NS * 36 + N * 8, dz = gam + 2 * NS * nck, kff = dz + NS * 10, Kl = kff + N * 4, Ginv = Kl + N * 16, hv = Ginv + N * 8, tile = hv + N * 8;
            CHECK(l.gt == NS * 10 && l.pv == NS * 28 && l.gam == gam && l.dz == dz && l.kff == kff && l.Kl == Kl && l.Ginv == Ginv && l.Prb == hv && l.tile == tile &&
                  l.hc == tile + 136 && (!path || l.ha == l.hc + NS * 2), "factor sweep offsets, path %d uni %d N %d", path, uni, N);
            CHECK(qp_lds_ric_agrees(N, c), "qp_lds_ric against the layout, path %d uni %d N %d", path, uni, N);
            // ---- reaches against a replay of the fetches ----
            Hull lv, lf, vv, vf;
            {
                int qe = l.Prb + (N - 1) * 8, qo = l.Prb + (N - 2) * 8, be = l.pv + (N - 1) * 8, bo = l.pv + (N - 2) * 8;      // lanes w, g = 0..7 on top
                replay(-1, N, SWEEP_RING, SWEEP_DL, [&](int, bool odd) {
                    int &q = odd ? qo : qe, &b = odd ? bo : be;
                    lv.word(q); lv.word(q + 7); lv.word(b); lv.word(b + 7);
                    q -= 16; b -= 16;
                });
                int ce = l.dz + 10, co = l.dz + 20;
                lf.word(l.dz);
                replay(+1, N, SWEEP_RING, SWEEP_DL, [&](int, bool odd) { int &cc = odd ? co : ce; lf.word(cc); lf.word(cc + 7); cc += 20; });
                replay(-1, N, QP_V1_RING, QP_V1_DL, [&](int k, bool) { vv.word(l.Prb + k * 8); vv.word(l.Prb + k * 8 + 7); vv.word(l.pv + k * 8); vv.word(l.pv + k * 8 + 7); });
                vf.word(l.dz);
                replay(+1, N, QP_V1_RING, QP_V1_DL, [&](int k, bool) { vf.word(l.dz + (k + 1) * 10); vf.word(l.dz + (k + 1) * 10 + 7); });
            }
            CHECK(lv.is(qp_reach_lean_vector(l, N, SWEEP_RING, SWEEP_DL)) && lf.is(qp_reach_lean_forward(l, N, SWEEP_RING, SWEEP_DL)), "lean reaches, N %d", N);
            CHECK(vv.is(qp_reach_v1_vector(l, N)) && vf.is(qp_reach_v1_forward(l, N)), "earlier form's reaches, N %d", N);
            // ---- inside the block ----
            CHECK(qp_factor_inside(l, N, c.nck), "factor stage / block reductions, path %d uni %d N %d", path, uni, N);
            CHECK(qp_sweeps_inside(l, N, true, SWEEP_RING, SWEEP_DL), "lean sweeps, path %d uni %d N %d", path, uni, N);
            const bool v1 = qp_sweeps_inside(l, N, false, 0, 0);
            CHECK(v1 == (N >= 4), "earlier form, path %d uni %d N %d", path, uni, N);
            if (!v1) {
                const int lo = qp_reach_v1_vector(l, N).lo;
                std::printf("path %d uni %d N %d: the earlier form's vector sweep reaches word %d\n", path, uni, N, lo);
                CHECK(qp_inside(qp_reach_v1_forward(l, N), 0, l.total), "the forward sweep stays inside");
                CHECK(lo == (N == 2 ? -60 : -24), "%d", lo);
            }
        }
    CHECK(qp_lds(2, qp_lds_class(0, true)).total == 744 && qp_lds(40, qp_lds_class(0, true)).total == 5076, "all-hard UNI at N = 2 and N = 40");
    // k_steps' guests
    CHECK(steps_lds_doubles(744, 0, true).total() == 744 && !steps_lds_doubles(744, 0, true).guests_fit(), "short horizons do not hold the integrator's 55 x 64 words");
    CHECK(steps_lds_doubles(5076, 1989, true).total() == 5076 && steps_lds_doubles(5076, 1989, true).guests_fit() && steps_lds_doubles(744, 1989, false).total() == 1989, "guests");
    if (fails) std::printf("%d checks failed\n", fails);
    else std::printf("qp_lds: all checks passed\n");
    return fails != 0;
}
