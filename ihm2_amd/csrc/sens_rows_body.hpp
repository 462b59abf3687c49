// sens_rows_body.hpp -- the constraint rows at xbar that the x0 sensitivities, the adjoint, the slack fold and the penalty gradients all
// differentiate: the row gradients of the track rows and the a_lat row (hc, ha), rcoef, and the walk over the slot table that evaluates
// every row at xbar (cz), the row times the step (rdz) and the multiplier, slack and gap of its lower and its upper side.
// A code fragment, not a header (no include guard, no namespace, no function of its own; NOTES.md R5.6, R23): sens_factor_body.hpp
// (sens_body, k_adj), k_slack_fold (kernels_slackseed.hip) and k_penalty_grad (kernels_penaltygrad.hip) #include it behind their LDS
// carve-up and early return, so that a row is written here and nowhere else.
//   Expects in scope: a (const SensArgs &), b, bs, lane, N, NS and the LDS pointers hc (NS*2), ha (NS*4).
//   Leaves in scope: xb, ubb, xo, uo, lamb, slkb, lamab, slkab, slb, sub, w_R, w_L, rcoef -- include it once per function body.  It
//   ends behind the hand-off that follows the walk: hc, ha and whatever the hooks stored are visible to every lane.
// Hooks, statement macros the includer defines before the #include and undefines after it (empty where it has nothing to do):
//   SENS_ROWS_CLEAR                  the lane's share of zeroing the includer's tables, in front of the first hand-off.
//   SENS_ROWS_SLOT_OPEN(s)           entry s of the slot table is in use (slot_kc[s] >= 0); nothing of its row is evaluated yet, so a
//                                    `continue` here skips the slot at no cost.
//   SENS_ROWS_SLOT_BEGIN(s)          k, c, cz, rdz, lb, ub of the slot are in scope; the includer's locals for its two sides.
//   SENS_ROWS_SIDE(k, c, up, lm, gap, sl)   once per side with a finite bound (up = 0: lower, 1: upper), inside a block of its own.
//                                    lm, sl: the expressions that load the side's multiplier and slack -- text, evaluated where and if
//                                    the includer writes them; gap: the side's primal gap without the slack.
//   SENS_ROWS_SLOT_END(k, c)         behind the two sides.
#if !defined(SENS_ROWS_CLEAR) || !defined(SENS_ROWS_SLOT_OPEN) || !defined(SENS_ROWS_SLOT_BEGIN) || !defined(SENS_ROWS_SIDE) || !defined(SENS_ROWS_SLOT_END)
#error "define SENS_ROWS_CLEAR, SENS_ROWS_SLOT_OPEN, SENS_ROWS_SLOT_BEGIN, SENS_ROWS_SIDE and SENS_ROWS_SLOT_END before including sens_rows_body.hpp"
#endif
    const double *xb = a.xbar + bs * NS * 8, *ubb = a.ubar + bs * N * 2;
    const double *xo = a.x + bs * NS * 8, *uo = a.u + bs * N * 2;
    const double *lamb = a.lam + bs * NS * 28, *slkb = a.slk + bs * NS * 28;
    const double *lamab = a.lam_a + bs * NS * 2, *slkab = a.slk_a + bs * NS * 2;
    const double *slb = a.slot_lb + bs * a.sl_bs, *sub = a.slot_ub + bs * a.sl_bs;
    // the slots' slack penalties zw, Zw, behind the bounds, for the hooks: the base is formed where it is read, wave-uniform, and not kept beside
    // slb / sub (the persistent loop's twin holds no register for it through the walk)
#define SENS_ROWS_ZW(s) ((a.slot_lb + (bs * a.sl_bs + a.nslots))[s])
#define SENS_ROWS_ZZ(s) ((a.slot_ub + (bs * a.sl_bs + a.nslots))[s])

    // ---- row gradients of the nonlinear rows at xbar, the includer's tables zeroed ----
    double w_R = 0.0, w_L = 0.0;
    if (a.path) {
        const int trk = a.track_id[b];
        w_R = a.widths[trk * 2 + 0]; w_L = a.widths[trk * 2 + 1];
    }
    for (int k = lane; k < NS; k += 64) {
        // the track rows as the QP forms them (kernels_qp.hip: qp_wave_body), stages 1..N
        const double psi = xb[k * 8 + 2], sgn = (psi > 0.0) - (psi < 0.0);
        const double dfoot = -0.5 * a.car_L * cos(fabs(psi)) * sgn, dlat = -0.5 * a.car_W * sin(psi);
        hc[k * 2 + 0] = (a.path && k >= 1) ? dfoot + dlat : 0.0;
        hc[k * 2 + 1] = (a.path && k >= 1) ? -dfoot + dlat : 0.0;
        double g4[4] = {0.0, 0.0, 0.0, 0.0};
        if (a.alat && k >= 1 && k < N) ihm2::alat_eval(xb[k * 8 + 3], xb[k * 8 + 4], xb[k * 8 + 6], xb[k * 8 + 7], g4);
#pragma unroll
        for (int q = 0; q < 4; q++) ha[k * 4 + q] = g4[q];
    }
    SENS_ROWS_CLEAR
    WSYNC();

    // coefficient of row c of stage k on the variable j of z_k = (dx_k, du_k)
    auto rcoef = [&](int k, int c, int j) -> double {
        if (c < 10) return (j == c) ? 1.0 : 0.0;
        if (c < 12) return a.CD[((size_t)k * 2 + (c - 10)) * 10 + j];
        if (c < 14) return (j == 1) ? ((c == 12) ? 1.0 : -1.0) : (j == 2) ? hc[k * 2 + (c - 12)] : 0.0;
        return (j == 3) ? ha[k * 4] : (j == 4) ? ha[k * 4 + 1] : (j == 6) ? ha[k * 4 + 2] : (j == 7) ? ha[k * 4 + 3] : 0.0;
    };

    // ---- the walk: every entry of the slot table on the lane that owns it in the QP (a split row's halves share a lane: no race) ----
    for (int s = lane; s < a.nslots; s += 64) {
        const int kc = a.slot_kc[s];
        if (kc < 0) continue;
        SENS_ROWS_SLOT_OPEN(s)
        const int k = kc >> 4, c = kc & 15;
        // row value at xbar (as the QP forms it) and the row times the step
        double cz, rdz = 0.0;
        if (c < 8) cz = xb[k * 8 + c];
        else if (c < 10) cz = ubb[k * 2 + c - 8];
        else if (c == 14) {
            double g4[4];
            cz = ihm2::alat_eval(xb[k * 8 + 3], xb[k * 8 + 4], xb[k * 8 + 6], xb[k * 8 + 7], g4);
        } else if (c >= 12) {
            const double n = xb[k * 8 + 1], psi = xb[k * 8 + 2];
            const double foot = -0.5 * a.car_L * sin(fabs(psi)), lat = 0.5 * a.car_W * cos(psi);
            cz = (c == 12) ? n + foot + lat - w_R : -n - foot + lat - w_L;
        } else {
            cz = 0.0;
            for (int j = 0; j < 8; j++) cz = fma(a.CD[((size_t)k * 2 + (c - 10)) * 10 + j], xb[k * 8 + j], cz);
            cz = fma(a.CD[((size_t)k * 2 + (c - 10)) * 10 + 8], ubb[k * 2 + 0], cz);
            cz = fma(a.CD[((size_t)k * 2 + (c - 10)) * 10 + 9], ubb[k * 2 + 1], cz);
        }
        for (int j = 0; j < 10; j++) {
            const double dzj = (j < 8) ? xo[k * 8 + j] - xb[k * 8 + j] : (k < N) ? uo[k * 2 + j - 8] - ubb[k * 2 + j - 8] : 0.0;
            rdz = fma(rcoef(k, c, j), dzj, rdz);
        }
        const double lb = slb[s], ub = sub[s];
        SENS_ROWS_SLOT_BEGIN(s)
        if (sfin(lb)) {
            SENS_ROWS_SIDE(k, c, 0, (c == 14) ? lamab[k * 2] : lamb[k * 28 + c], rdz - (lb - cz), (c == 14) ? slkab[k * 2] : slkb[k * 28 + c])
        }
        if (sfin(ub)) {
            SENS_ROWS_SIDE(k, c, 1, (c == 14) ? lamab[k * 2 + 1] : lamb[k * 28 + 14 + c], (ub - cz) - rdz, (c == 14) ? slkab[k * 2 + 1] : slkb[k * 28 + 14 + c])
        }
        SENS_ROWS_SLOT_END(k, c)
    }
    WSYNC();
#undef SENS_ROWS_ZW
#undef SENS_ROWS_ZZ
