// check_fkin6_algebra.cpp -- the two rewrites of fkin6's arithmetic as host code (tests/test_fkin6_algebra.py builds this file with the address and
// undefined-behaviour sanitizers and runs it):
//  (a) the steering block of fkin6_eval (csrc/model.hpp) without the tangent: cos(beta), sin(beta), beta' and beta'' from sin(delta), cos(delta)
//      and ONE reciprocal, against beta = atan(c tan(delta)) in long double, next to the form it replaces (td = sd / cd, den = 1 + c^2 td^2);
//  (b) rows 2 and 5 of the Jacobian applied to a sensitivity column in factored form (csrc/device_steps.hpp: fkin6_factored_row) against the
//      dense row products of sens_col_stage.
// The formulas are copies: model.hpp and device_steps.hpp are device code.  The test compares the copied statements with the headers' text.
// usage: check_fkin6_algebra [delta ...]      (further steering angles for the grid of (a))
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

constexpr double k_m = 230.0, k_lR = 0.7853, k_wheelbase = 1.5706, k_rwd = k_lR / k_wheelbase;
constexpr double k_Cm0 = 4.950, k_Cr0 = 297.030, k_Cr1 = 16.665, k_Cr2 = 0.6784, k_tT = 1e-3, k_tdelta = 0.02;

constexpr unsigned JX_MASK[2][8] = {{0x1Fu, 0x1Cu, 0x3Fu, 0xD8u, 0xC8u, 0xC8u, 0x40u, 0x80u},
                                    {0x1Fu, 0x1Cu, 0x3Fu, 0xF8u, 0xF8u, 0xF8u, 0x40u, 0x80u}};
constexpr unsigned JU_MASK[2][8] = {{0u, 0u, 0u, 2u, 2u, 2u, 1u, 2u}, {0u, 0u, 0u, 0u, 0u, 0u, 1u, 2u}};
constexpr unsigned S_COL_MASK[2][10] = {{0x07u, 0x07u, 0x07u, 0x3Fu, 0x3Fu, 0x27u, 0x7Fu, 0xBFu, 0x7Fu, 0xBFu},
                                        {0x07u, 0x07u, 0x07u, 0x3Fu, 0x3Fu, 0x3Fu, 0x7Fu, 0xBFu, 0x7Fu, 0xBFu}};
constexpr int FKIN6_F_ROW2 = 2, FKIN6_F_KAP = 6, FKIN6_F_DKS = 7, FKIN6_F_ROW5 = 5, FKIN6_F_DBD_DD = 0, FKIN6_F_DBD_DU = 1;
constexpr int FKIN6_JAC_NONE = 0, FKIN6_JAC_DENSE = 1, FKIN6_JAC_FACTORED = 2;

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

double tanh_e(double y)
{
    const double t = std::exp(-2.0 * std::fabs(y));
    return std::copysign((1.0 - t) / (1.0 + t), y);
}

// ---- (a) ----
struct Steer { double cb, sb, bp, bpp; };

// the block as it stands in model.hpp (the statements between the markers are the header's)
Steer steer_new(double sd, double cd)
{
    const double c = k_rwd;
    // [steering block]
    const double hyp2 = 1.0 / (cd * cd + c * c * sd * sd);
    const double hyp = sqrt(hyp2);
    const double cb = cd * hyp, sb = c * sd * hyp;
    const double bp = c * hyp2;                           // d beta / d delta
    // [end]
    const double bpp = (2.0 * c * (1.0 - c * c)) * (sd * cd) * (hyp2 * hyp2);
    return {cb, sb, bp, bpp};
}
// the block it replaces
Steer steer_old(double sd, double cd)
{
    const double c = k_rwd;
    const double td = sd / cd;
    const double hyp = 1.0 / sqrt(cd * cd + c * c * sd * sd);
    const double cb = cd * hyp, sb = c * sd * hyp;
    const double den = 1.0 + c * c * td * td;
    const double bp = c * (1.0 + td * td) / den;
    const double bpp = 2.0 * c * td * (1.0 + td * td) * (1.0 - c * c) / (den * den);
    return {cb, sb, bp, bpp};
}
// python/models.py:261-284 in long double: beta = atan(c tan(delta)) and its two derivatives in delta
void steer_ref(double delta, long double (&r)[4])
{
    const long double c = (long double)k_lR / (long double)k_wheelbase, t = tanl((long double)delta);
    const long double beta = atanl(c * t), den = 1.0L + c * c * t * t;
    r[0] = cosl(beta);
    r[1] = sinl(beta);
    r[2] = c * (1.0L + t * t) / den;
    r[3] = 2.0L * c * t * (1.0L + t * t) * (1.0L - c * c) / (den * den);
}
double rel_err(double v, long double ref)
{
    if (ref == 0.0L) return v == 0.0 ? 0.0 : HUGE_VAL;
    return (double)fabsl(((long double)v - ref) / ref);
}

void check_steering(const std::vector<double> &extra)
{
    std::vector<double> grid;
    const int n = 200000;
    for (int i = 0; i <= n; i++) grid.push_back(-1.55 + 3.1 * i / n);
    grid.push_back(0.0);
    for (double d : extra) grid.push_back(d);
    double worst_new[4] = {0, 0, 0, 0}, worst_old[4] = {0, 0, 0, 0};
    for (double delta : grid) {
        CHECK(std::fabs(delta) <= 1.55, "delta %g outside the grid's range", delta);
        const double sd = std::sin(delta), cd = std::cos(delta);
        const Steer a = steer_new(sd, cd), b = steer_old(sd, cd);
        long double r[4];
        steer_ref(delta, r);
        const double va[4] = {a.cb, a.sb, a.bp, a.bpp}, vb[4] = {b.cb, b.sb, b.bp, b.bpp};
        for (int q = 0; q < 4; q++) {
            worst_new[q] = std::max(worst_new[q], rel_err(va[q], r[q]));
            worst_old[q] = std::max(worst_old[q], rel_err(vb[q], r[q]));
        }
    }
    const char *names[4] = {"cos(beta)", "sin(beta)", "beta'", "beta''"};
    for (int q = 0; q < 4; q++) {
        std::printf("steering %-9s worst relative error on %zu angles: new %.3e  earlier %.3e\n", names[q], grid.size(), worst_new[q], worst_old[q]);
        CHECK(worst_new[q] <= 2.0 * worst_old[q], "%s: %.3e against twice %.3e", names[q], worst_new[q], worst_old[q]);
    }
}

// ---- (b) ----
// fkin6_eval of model.hpp with sin, cos of libm and the curvature and its slope as arguments; the Jacobian block is the header's text
template <int WITH_JAC>
void fkin6_host(const double (&x)[8], double u_T, double u_delta, double kap, double dk, double (&f)[8], double (&J)[8][10])
{
    const double c = k_rwd;
    const double n = x[1], psi = x[2], v_x = x[3], v_y = x[4], r = x[5], T = x[6], delta = x[7];
    const double delta_dot = (u_delta - delta) * (1.0 / k_tdelta);
    const double T_dot = (u_T - T) * (1.0 / k_tT);
    const double F_motor = k_Cm0 * T;
    const double sg = tanh_e(10.0 * v_x);
    const double poly = k_Cr0 + k_Cr1 * v_x + k_Cr2 * v_x * v_x;
    const double F_drag = -poly * sg;
    const double F_Rx = 0.5 * F_motor + F_drag, F_Fx = 0.5 * F_motor;
    const double sd = std::sin(delta), cd = std::cos(delta);
    const double hyp2 = 1.0 / (cd * cd + c * c * sd * sd);
    const double hyp = sqrt(hyp2);
    const double cb = cd * hyp, sb = c * sd * hyp;
    const double bp = c * hyp2;                           // d beta / d delta
    const double beta_dot = bp * delta_dot;
    const double cdb = cd * cb + sd * sb, sdb = sd * cb - cd * sb;      // cos / sin (delta - beta)
    const double v_dot = (F_Rx * cb + F_Fx * cdb) * (1.0 / k_m);
    const double sp = std::sin(psi), cp = std::cos(psi);
    const double num = v_x * cp - v_y * sp;
    const double dn = 1.0 + kap * n;
    const double inv_dn = 1.0 / dn;
    const double s_dot = num * inv_dn;
    const double v_y_dot = v_dot * sb + beta_dot * v_x;
    f[0] = s_dot;
    f[1] = v_x * sp + v_y * cp;
    f[2] = r - kap * s_dot;
    f[3] = v_dot * cb - beta_dot * v_y;
    f[4] = v_y_dot;
    f[5] = k_lR * v_y_dot - beta_dot;
    f[6] = T_dot;
    f[7] = delta_dot;
    // [jacobian block]
    if (WITH_JAC) {
        const double dFdrag = -(k_Cr1 + 2.0 * k_Cr2 * v_x) * sg - poly * 10.0 * (1.0 - sg * sg);
        const double bpp = (2.0 * c * (1.0 - c * c)) * (sd * cd) * (hyp2 * hyp2);
        const double dbd_dd = bpp * delta_dot - bp * (1.0 / k_tdelta);
        const double dbd_du = bp * (1.0 / k_tdelta);
        const double dv_dvx = dFdrag * cb * (1.0 / k_m);
        const double dv_dT = 0.5 * k_Cm0 * (cb + cdb) * (1.0 / k_m);
        const double dv_dd = (-F_Rx * sb * bp - F_Fx * sdb * (1.0 - bp)) * (1.0 / k_m);
        const double q = -s_dot * inv_dn;          // d s_dot / d (kappa n)
        J[0][0] = q * dk * n;
        J[0][1] = q * kap;
        J[0][2] = (-v_x * sp - v_y * cp) * inv_dn;
        J[0][3] = cp * inv_dn;
        J[0][4] = -sp * inv_dn;
        J[1][2] = num;
        J[1][3] = sp;
        J[1][4] = cp;
        if (WITH_JAC == FKIN6_JAC_FACTORED) {
            J[FKIN6_F_ROW2][FKIN6_F_KAP] = kap;
            J[FKIN6_F_ROW2][FKIN6_F_DKS] = (dk * num) * inv_dn;
            J[FKIN6_F_ROW5][FKIN6_F_DBD_DD] = dbd_dd;
            J[FKIN6_F_ROW5][FKIN6_F_DBD_DU] = dbd_du;
        } else {
            J[2][0] = -dk * s_dot - kap * J[0][0];
            J[2][1] = -kap * J[0][1];
            J[2][2] = -kap * J[0][2];
            J[2][3] = -kap * J[0][3];
            J[2][4] = -kap * J[0][4];
            J[2][5] = 1.0;
        }
        J[3][3] = dv_dvx * cb;
        J[3][4] = -beta_dot;
        J[3][6] = dv_dT * cb;
        J[3][7] = dv_dd * cb - v_dot * sb * bp - dbd_dd * v_y;
        J[3][9] = -dbd_du * v_y;
        J[4][3] = dv_dvx * sb + beta_dot;
        J[4][6] = dv_dT * sb;
        J[4][7] = dv_dd * sb + v_dot * cb * bp + dbd_dd * v_x;
        J[4][9] = dbd_du * v_x;
        if (WITH_JAC != FKIN6_JAC_FACTORED) {
            J[5][3] = k_lR * J[4][3];
            J[5][6] = k_lR * J[4][6];
            J[5][7] = k_lR * J[4][7] - dbd_dd;
            J[5][9] = k_lR * J[4][9] - dbd_du;
        }
        J[6][6] = -1.0 / k_tT;
        J[6][8] = 1.0 / k_tT;
        J[7][7] = -1.0 / k_tdelta;
        J[7][9] = 1.0 / k_tdelta;
    }
    // [end]
}

// device_steps.hpp's function, its body the header's text
template <int COL>
double fkin6_factored_row(int i, const double (&J)[8][10], const double (&dX)[8], const double (&dK)[8])
// [factored row]
{
    constexpr unsigned cm = S_COL_MASK[0][COL];
    double acc = 0.0;
    if (i == 2) {
        if ((cm >> 5) & 1u) acc = dX[5];
        acc = fma(-J[FKIN6_F_ROW2][FKIN6_F_DKS], dX[0], acc);
        acc = fma(-J[FKIN6_F_ROW2][FKIN6_F_KAP], dK[0], acc);
    } else {
        if (COL == 9) acc = -J[FKIN6_F_ROW5][FKIN6_F_DBD_DU];
        if ((cm >> 4) & 1u) acc = fma(k_lR, dK[4], acc);
        if ((cm >> 7) & 1u) acc = fma(-J[FKIN6_F_ROW5][FKIN6_F_DBD_DD], dX[7], acc);
    }
    return acc;
}
// [end]

// the row loop of sens_col_stage<0, COL, FACTORED> on a given dX (rows 0..5: what the factored rows read and write)
template <int COL, bool FACTORED>
void stage_rows(const double (&J)[8][10], const double (&dX)[8], double (&dK)[8])
{
    constexpr unsigned cm = S_COL_MASK[0][COL];
    for (int i = 0; i < 6; i++) {
        if (!((cm >> i) & 1u)) continue;
        if (FACTORED && (i == 2 || i == 5)) { dK[i] = fkin6_factored_row<COL>(i, J, dX, dK); continue; }
        double acc = 0.0;
        if constexpr (COL >= 8) { if ((JU_MASK[0][i] >> (COL - 8)) & 1u) acc = J[i][COL]; }
        for (int l = 0; l < 8; l++)
            if (((JX_MASK[0][i] & cm) >> l) & 1u) acc = fma(J[i][l], dX[l], acc);
        dK[i] = acc;
    }
}

struct Rng {          // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni(double a, double b) { return a + (b - a) * (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

double worst_ulp[2] = {0.0, 0.0};
double ulp_of(double s) { return std::nextafter(s, HUGE_VAL) - s; }

// The scale of the comparison: the sum of the absolute values of the terms in their finest form, i.e. with the dense entries that are
// differences themselves taken apart -- J[2][0] = -kappa' s_dot - kappa J[0][0], J[5][7] = l_R J[4][7] - dbd_dd, J[5][9] = l_R J[4][9] - dbd_du.
// The dense form rounds those entries at the size of their parts (l_R dbd_dd v_x and dbd_dd cancel at v_x = 1 / l_R), so neither form is
// defined more finely than an ulp of the parts.
template <int COL>
void check_column(const double (&Jd)[8][10], const double (&Jf)[8][10], const double (&dX)[8], int draw)
{
    constexpr unsigned cm = S_COL_MASK[0][COL];
    double dKd[8], dKf[8];
    for (int i = 0; i < 8; i++) dKd[i] = dKf[i] = NAN;          // a row outside the mask is never read
    stage_rows<COL, false>(Jd, dX, dKd);
    stage_rows<COL, true>(Jf, dX, dKf);
    for (int i : {0, 1, 3, 4})
        if ((cm >> i) & 1u) CHECK(dKd[i] == dKf[i], "column %d row %d draw %d: the rows that stay dense differ", COL, i, draw);
    const double kap = Jf[FKIN6_F_ROW2][FKIN6_F_KAP], dks = Jf[FKIN6_F_ROW2][FKIN6_F_DKS];
    double sum2 = std::fabs(dks * dX[0]) + (((cm >> 5) & 1u) ? std::fabs(dX[5]) : 0.0);
    for (int l = 0; l < 5; l++)
        if (((JX_MASK[0][0] & cm) >> l) & 1u) sum2 += std::fabs(kap * Jd[0][l] * dX[l]);
    const double u2 = std::fabs(dKd[2] - dKf[2]) / ulp_of(sum2);
    worst_ulp[0] = std::max(worst_ulp[0], sum2 > 0.0 ? u2 : 0.0);
    CHECK(std::fabs(dKd[2] - dKf[2]) <= 8.0 * ulp_of(sum2), "column %d row 2 draw %d: %.17g against %.17g, %.2f ulp of %.3g", COL, draw, dKf[2], dKd[2], u2, sum2);
    if ((cm >> 5) & 1u) {
        const double dbd_dd = Jf[FKIN6_F_ROW5][FKIN6_F_DBD_DD], dbd_du = Jf[FKIN6_F_ROW5][FKIN6_F_DBD_DU];
        double sum5 = 0.0;
        for (int l = 0; l < 8; l++)
            if (((JX_MASK[0][4] & cm) >> l) & 1u) sum5 += std::fabs(k_lR * Jd[4][l] * dX[l]);
        if ((cm >> 7) & 1u) sum5 += std::fabs(dbd_dd * dX[7]);
        if (COL == 9) sum5 += std::fabs(k_lR * Jd[4][9]) + std::fabs(dbd_du);
        const double u5 = std::fabs(dKd[5] - dKf[5]) / ulp_of(sum5);
        if (sum5 > 0.0) worst_ulp[1] = std::max(worst_ulp[1], u5);
        CHECK(std::fabs(dKd[5] - dKf[5]) <= 8.0 * ulp_of(sum5), "column %d row 5 draw %d: %.17g against %.17g, %.2f ulp of %.3g", COL, draw, dKf[5], dKd[5], u5, sum5);
    }
}

void check_factored_rows()
{
    Rng rng{20241019};
    const int draws = 10000;
    for (int d = 0; d < draws; d++) {
        // states over the ranges of tests/edge_states.py: |delta| <= 1.5, v_x from reverse to 40 m/s, 1 + kappa n >= 0.5
        double x[8] = {0.0, rng.uni(-1.5, 1.5), rng.uni(-3.2, 3.2), rng.uni(-3.0, 40.0), rng.uni(-2.0, 2.0), rng.uni(-2.0, 2.0), rng.uni(-300.0, 300.0), rng.uni(-1.5, 1.5)};
        if (d % 4 == 0) x[3] = rng.uni(-0.1, 0.1);                                // around the tanh's transition
        if (d % 4 == 1) x[3] = 1.0 / k_lR * (1.0 + rng.uni(-1e-6, 1e-6));         // where l_R J[4][7] and dbd_dd cancel in the dense J[5][7]
        const double u_T = rng.uni(-400.0, 400.0), u_delta = rng.uni(-1.5, 1.5);
        const double kap = rng.uni(-0.3, 0.3), dk = rng.uni(-0.2, 0.2);
        double f1[8], f2[8], Jd[8][10], Jf[8][10];
        for (auto &row : Jd) for (double &v : row) v = NAN;                      // never written, never read
        for (auto &row : Jf) for (double &v : row) v = NAN;
        fkin6_host<FKIN6_JAC_DENSE>(x, u_T, u_delta, kap, dk, f1, Jd);
        fkin6_host<FKIN6_JAC_FACTORED>(x, u_T, u_delta, kap, dk, f2, Jf);
        for (int i = 0; i < 8; i++) CHECK(f1[i] == f2[i], "draw %d: xdot differs between the forms", d);
        int written = 0;
        for (int i = 0; i < 8; i++)
            for (int j = 0; j < 10; j++) {
                const bool dense = (j < 8) ? ((JX_MASK[0][i] >> j) & 1u) : ((JU_MASK[0][i] >> (j - 8)) & 1u);
                CHECK(dense == !std::isnan(Jd[i][j]), "draw %d: dense entry (%d, %d) against the masks", d, i, j);
                written += !std::isnan(Jf[i][j]);
                if (i != 2 && i != 5) CHECK(std::isnan(Jd[i][j]) ? std::isnan(Jf[i][j]) : Jd[i][j] == Jf[i][j], "draw %d: entry (%d, %d) differs between the forms", d, i, j);
            }
        CHECK(written == 31 - 10 + 4, "draw %d: the factored form wrote %d entries", d, written);
        double dX[8];
        for (double &v : dX) v = rng.uni(-1.0, 1.0) * std::pow(10.0, rng.uni(-3.0, 3.0));
#define COL(c) check_column<c>(Jd, Jf, dX, d);
        COL(0) COL(1) COL(2) COL(3) COL(4) COL(5) COL(6) COL(7) COL(8) COL(9)
#undef COL
    }
    std::printf("factored rows: %d draws x 10 columns, worst difference %.2f ulp of the terms' sum in row 2, %.2f in row 5 (bound 8)\n", draws, worst_ulp[0], worst_ulp[1]);
}

}  // namespace

int main(int argc, char **argv)
{
    std::vector<double> extra;
    for (int i = 1; i < argc; i++) extra.push_back(std::strtod(argv[i], nullptr));
    check_steering(extra);
    check_factored_rows();
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
