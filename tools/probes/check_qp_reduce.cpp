// The packed wave reductions of ihm2_amd/csrc/qp_reduce.hpp run on 64 software lanes, as a program of its own:
//   * the exchange steps: what the DPP controls and the row / half swaps do, decoded here from their definitions, is qr_src_lane; every step is a
//     permutation of the lanes that stays inside the class the header says it keeps;
//   * ownership: the butterfly is replayed on SETS (which lanes' inputs of which value a lane's registers hold); after every step a lane holds
//     a part of value v exactly when qr4_owns / qr2_owns says so, and after the last step the lanes of qr4_class_of(v) hold all 64 inputs of v;
//   * values: the same replay on doubles with fmax / fmin and the NaN ballot, against the sequential definitions the kernels used before
//     (nanmax over the lanes in order, fmin over the lanes in order), bit for bit: the unique maximum in each of the 4 x 64 places, a NaN in each
//     of them, 10 000 random draws with inf, 0 and denormals; and the claims of the header's argument -- non-negative operands, step bounds
//     in (0, 1] that are never NaN even when their inputs are.
// Build: g++ -std=c++17 -I ihm2_amd/csrc tools/probes/check_qp_reduce.cpp   (also with -fsanitize=address,undefined)
#include <array>
#include <bitset>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "qp_reduce.hpp"

using namespace ihm2;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; if (fails < 50) { std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }

// ---- what the hardware's exchanges do (from their definitions, not from the header) ----
// DPP control -> source lane: quad_perm 0x00..0xFF (two bits per lane of the quad), row_ror:n 0x121..0x12F (lane i of a row of 16 takes lane i - n)
static int dpp_src(int ctrl, int lane)
{
    if (ctrl >= 0 && ctrl <= 0xFF) return (lane & ~3) | ((ctrl >> (2 * (lane & 3))) & 3);
    if (ctrl >= 0x121 && ctrl <= 0x12F) return (lane & ~15) | ((lane - (ctrl & 15)) & 15);
    return -1;
}
// v_permlane16_swap / v_permlane32_swap of a register with itself: one result is the lane's own value, the other that of lane ^ 16 / lane ^ 32
static int swap_src(int step, int lane) { return lane ^ (step == 4 ? 16 : 32); }

// ---- the butterfly of the header on a lane type T with a symmetric op: the device code's statements, lane by lane ----
template <typename T> using Wave = std::array<T, 64>;
template <typename T> static Wave<T> lane_exchange(int step, const Wave<T> &v)
{
    Wave<T> r;
    for (int l = 0; l < 64; l++) r[l] = v[qr_src_lane(step, l)];
    return r;
}
template <typename T, typename OP> static void tail(Wave<T> &k, OP op)
{
    for (int step = 2; step < QR_STEPS; step++) {
        const Wave<T> got = lane_exchange(step, k);
        for (int l = 0; l < 64; l++) k[l] = op(k[l], got[l]);
    }
}
template <typename T, typename OP, typename SEE> static void max4(Wave<T> &a, Wave<T> &b, Wave<T> &c, Wave<T> &d, OP op, SEE see)
{
    Wave<T> k0, k1, s0, s1, k, s;
    Wave<int> v0, v1, vk;       // which value a register holds
    for (int l = 0; l < 64; l++) {
        const bool p = !qr4_owns(1, l & 3, 0);
        k0[l] = p ? c[l] : a[l]; k1[l] = p ? d[l] : b[l]; s0[l] = p ? a[l] : c[l]; s1[l] = p ? b[l] : d[l];
        v0[l] = p ? 2 : 0; v1[l] = p ? 3 : 1;
    }
    const Wave<T> g0 = lane_exchange(0, s0), g1 = lane_exchange(0, s1);
    for (int l = 0; l < 64; l++) { k0[l] = op(k0[l], g0[l]); k1[l] = op(k1[l], g1[l]); }
    see(1, k0, v0); see(1, k1, v1);
    for (int l = 0; l < 64; l++) {
        const bool q = !qr4_owns(2, l & 3, v0[l]);
        k[l] = q ? k1[l] : k0[l]; s[l] = q ? k0[l] : k1[l]; vk[l] = q ? v1[l] : v0[l];
    }
    const Wave<T> g = lane_exchange(1, s);
    for (int l = 0; l < 64; l++) k[l] = op(k[l], g[l]);
    see(2, k, vk);
    tail(k, op);
    see(QR_STEPS, k, vk);
    for (int l = 0; l < 64; l++) {
        a[l] = k[dpp_src(qr_quad_bcast(qr4_class_of(0)), l)]; b[l] = k[dpp_src(qr_quad_bcast(qr4_class_of(1)), l)];
        c[l] = k[dpp_src(qr_quad_bcast(qr4_class_of(2)), l)]; d[l] = k[dpp_src(qr_quad_bcast(qr4_class_of(3)), l)];
    }
}
template <typename T, typename OP, typename SEE> static void min2(Wave<T> &a, Wave<T> &b, OP op, SEE see)
{
    Wave<T> k, s;
    Wave<int> vk;
    for (int l = 0; l < 64; l++) { const bool p = !qr2_owns(1, l & 1, 0); k[l] = p ? b[l] : a[l]; s[l] = p ? a[l] : b[l]; vk[l] = p ? 1 : 0; }
    Wave<T> g = lane_exchange(0, s);
    for (int l = 0; l < 64; l++) k[l] = op(k[l], g[l]);
    see(1, k, vk);
    g = lane_exchange(1, k);
    for (int l = 0; l < 64; l++) k[l] = op(k[l], g[l]);
    tail(k, op);
    see(QR_STEPS, k, vk);
    for (int l = 0; l < 64; l++) { a[l] = k[dpp_src(qr_quad_bcast(qr2_class_of(0)), l)]; b[l] = k[dpp_src(qr_quad_bcast(qr2_class_of(1)), l)]; }
}

// ---- the definitions the packed forms must reproduce ----
static double nanmax(double a, double b) { return (a != a || b != b) ? std::numeric_limits<double>::quiet_NaN() : std::fmax(a, b); }
static double seq_nanmax(const Wave<double> &v) { double r = v[0]; for (int l = 1; l < 64; l++) r = nanmax(r, v[l]); return r; }
static double seq_min(const Wave<double> &v) { double r = v[0]; for (int l = 1; l < 64; l++) r = std::fmin(r, v[l]); return r; }
// today's one-value butterfly (xor 1, xor 2, mirror in 8, rotate by 8, the swaps) -- the order the kernels reduce in now
template <typename OP> static double old_butterfly(Wave<double> v, OP op)
{
    const int ctrl[4] = {0xB1, 0x4E, -1, 0x128};
    for (int step = 0; step < 6; step++) {
        Wave<double> g;
        for (int l = 0; l < 64; l++) g[l] = v[step == 2 ? ((l & ~7) | (7 - (l & 7))) : step < 4 ? dpp_src(ctrl[step], l) : swap_src(step, l)];
        for (int l = 0; l < 64; l++) v[l] = op(v[l], g[l]);
    }
    for (int l = 1; l < 64; l++) CHECK(bits(v[l]) == bits(v[0]), "today's butterfly: lane %d differs", l);
    return v[0];
}

// the norms as the kernel forms them: any_nan by ballot, maxima by fmax, result any_nan ? NAN : max
static void packed_norms(Wave<double> v[4], double out[4])
{
    bool any[4];
    for (int i = 0; i < 4; i++) { any[i] = false; for (int l = 0; l < 64; l++) any[i] |= v[i][l] != v[i][l]; }
    auto nosee = [](int, const Wave<double> &, const Wave<int> &) {};
    max4(v[0], v[1], v[2], v[3], [](double x, double y) { return std::fmax(x, y); }, nosee);
    for (int i = 0; i < 4; i++) {
        for (int l = 1; l < 64; l++) CHECK(bits(v[i][l]) == bits(v[i][0]) || any[i], "value %d: lane %d got another maximum", i, l);
        out[i] = any[i] ? std::numeric_limits<double>::quiet_NaN() : v[i][0];
    }
}
static void check_norms(const Wave<double> in[4], const char *what, int n)
{
    Wave<double> v[4] = {in[0], in[1], in[2], in[3]};
    double got[4];
    packed_norms(v, got);
    for (int i = 0; i < 4; i++) {
        const double want = seq_nanmax(in[i]), today = old_butterfly(in[i], nanmax);
        CHECK(bits(got[i]) == bits(want) && bits(today) == bits(want), "%s %d value %d: packed %a, today's butterfly %a, sequential %a", what, n, i, got[i], today, want);
    }
}
static void check_bounds(const Wave<double> &a, const Wave<double> &b, const char *what, int n)
{
    Wave<double> x = a, y = b;
    min2(x, y, [](double p, double q) { return std::fmin(p, q); }, [](int, const Wave<double> &, const Wave<int> &) {});
    const double wa = seq_min(a), wb = seq_min(b);
    for (int l = 0; l < 64; l++) CHECK(bits(x[l]) == bits(wa) && bits(y[l]) == bits(wb), "%s %d lane %d: packed (%a, %a), sequential (%a, %a)", what, n, l, x[l], y[l], wa, wb);
    CHECK(bits(old_butterfly(a, [](double p, double q) { return std::fmin(p, q); })) == bits(wa), "%s %d: today's butterfly against the sequential minimum", what, n);
}

int main()
{
    // ---- the steps ----
    for (int step = 0; step < QR_STEPS; step++) {
        std::bitset<64> hit;
        for (int l = 0; l < 64; l++) {
            const int s = qr_src_lane(step, l);
            CHECK(s >= 0 && s < 64, "step %d lane %d: source %d", step, l, s);
            if (s < 0 || s >= 64) continue;
            hit.set(s);
            CHECK(s == (step < 4 ? dpp_src(qr_dpp_ctrl(step), l) : swap_src(step, l)), "step %d lane %d: the header says lane %d, the instruction reads another", step, l, s);
            CHECK(qr4_step_fits(step, l) && qr2_step_fits(step, l), "step %d lane %d leaves its class", step, l);
        }
        CHECK(hit.all(), "step %d is no permutation", step);
        CHECK((step < 4) == (qr_dpp_ctrl(step) >= 0), "step %d: DPP control", step);
    }
    for (int c = 0; c < 4; c++) for (int l = 0; l < 64; l++) CHECK(dpp_src(qr_quad_bcast(c), l) == ((l & ~3) | c), "quad broadcast of lane %d", c);
    for (int v = 0; v < 4; v++) CHECK(qr4_value_of(qr4_class_of(v)) == v && qr4_owns(QR_STEPS, qr4_class_of(v), v), "value %d and its class", v);

    // ---- ownership: the replay on sets of (value, input lane) ----
    {
        using Set = std::bitset<256>;
        Wave<Set> in[4];
        for (int v = 0; v < 4; v++) for (int l = 0; l < 64; l++) in[v][l].set(v * 64 + l);
        auto see4 = [](int done, const Wave<Set> &k, const Wave<int> &vk) {
            for (int l = 0; l < 64; l++) {
                for (int v = 0; v < 4; v++) {
                    const bool holds = (k[l] >> (v * 64) & Set(~0ull)).any();
                    if (holds) CHECK(v == vk[l] && qr4_owns(done, l & 3, v), "after %d steps lane %d holds inputs of value %d", done, l, v);
                }
                CHECK(qr4_owns(done, l & 3, vk[l]), "after %d steps lane %d keeps value %d against the header", done, l, vk[l]);
                CHECK((int)k[l].count() == (done == QR_STEPS ? 64 : 1 << done), "after %d steps lane %d has %d inputs", done, l, (int)k[l].count());
                if (done >= 2) CHECK(vk[l] == qr4_value_of(l & 3), "lane %d reduces value %d", l, vk[l]);
            }
        };
        max4(in[0], in[1], in[2], in[3], [](Set x, Set y) { return x | y; }, see4);
        for (int v = 0; v < 4; v++) for (int l = 0; l < 64; l++) {
            Set all; for (int q = 0; q < 64; q++) all.set(v * 64 + q);
            CHECK(in[v][l] == all, "result %d in lane %d misses inputs or has foreign ones", v, l);
        }
        int owners[3][4] = {};
        for (int done = 1; done <= 2; done++) for (int cls = 0; cls < 4; cls++) for (int v = 0; v < 4; v++) owners[done][cls] += qr4_owns(done, cls, v);
        for (int cls = 0; cls < 4; cls++) CHECK(owners[1][cls] == 2 && owners[2][cls] == 1, "class %d keeps %d then %d values", cls, owners[1][cls], owners[2][cls]);

        Wave<Set> a, b;
        for (int l = 0; l < 64; l++) { a[l].set(l); b[l].set(64 + l); }
        auto see2 = [](int done, const Wave<Set> &k, const Wave<int> &vk) {
            for (int l = 0; l < 64; l++) {
                for (int v = 0; v < 2; v++) if ((k[l] >> (v * 64) & Set(~0ull)).any()) CHECK(v == vk[l] && qr2_owns(done, l & 1, v), "two values: after %d steps lane %d holds value %d", done, l, v);
                CHECK((int)k[l].count() == (done == QR_STEPS ? 64 : 2), "two values: after %d steps lane %d has %d inputs", done, l, (int)k[l].count());
            }
        };
        min2(a, b, [](Set x, Set y) { return x | y; }, see2);
        for (int l = 0; l < 64; l++) {
            Set wa, wb; for (int q = 0; q < 64; q++) { wa.set(q); wb.set(64 + q); }
            CHECK(a[l] == wa && b[l] == wb, "two values: results in lane %d", l);
        }
    }

    // ---- values ----
    std::mt19937_64 rng(20240611);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    auto draw = [&](bool special) -> double {      // non-negative, as everything the kernels reduce this way
        const int r = special ? (int)(rng() % 12) : 99;
        if (r == 0) return 0.0;
        if (r == 1) return std::numeric_limits<double>::infinity();
        if (r == 2) return std::numeric_limits<double>::denorm_min() * (double)(1 + rng() % 4096);
        if (r == 3) return std::numeric_limits<double>::min();
        return std::exp(60.0 * uni(rng) - 30.0);
    };
    int cases = 0;
    for (int pos = 0; pos < 4; pos++)
        for (int lane = 0; lane < 64; lane++) {
            Wave<double> v[4];
            for (auto &w : v) for (auto &x : w) x = draw(false);
            v[pos][lane] = 1e40;                                        // the unique maximum of its value
            check_norms(v, "maximum at", pos * 64 + lane);
            Wave<double> lo[2] = {v[0], v[1]};
            lo[pos & 1][lane] = 1e-40;                                  // the unique minimum
            check_bounds(lo[0], lo[1], "minimum at", pos * 64 + lane);
            v[pos][lane] = (lane & 1) ? std::numeric_limits<double>::quiet_NaN() : std::fabs(std::nan("0x5a5a"));      // (a payload must not come through)
            check_norms(v, "NaN at", pos * 64 + lane);
            cases += 3;
        }
    for (int n = 0; n < 10000; n++) {
        Wave<double> v[4];
        for (auto &w : v) for (auto &x : w) x = draw(true);
        if (n % 5 == 0) v[rng() % 4][rng() % 64] = std::numeric_limits<double>::quiet_NaN();
        if (n % 50 == 0) for (auto &x : v[rng() % 4]) x = std::numeric_limits<double>::quiet_NaN();        // a whole value of NaNs
        check_norms(v, "draw", n);
        // step bounds as the kernel forms them from max(-dt / t) and max(-dlam / lam): never NaN, in (0, 1] or 0 for an infinite ratio
        Wave<double> sa, sb;
        for (int l = 0; l < 64; l++) {
            const double ra = std::fmax(1.0, v[0][l]), rb = std::fmax(1.0, v[1][l]);        // fmax drops a NaN operand
            sa[l] = std::fmin(1.0, 1.0 / ra); sb[l] = std::fmin(1.0, 1.0 / rb);
            CHECK(sa[l] == sa[l] && sb[l] == sb[l] && sa[l] >= 0.0 && sa[l] <= 1.0 && !std::signbit(sa[l]) && !std::signbit(sb[l]), "draw %d lane %d: a step bound outside [0, 1]", n, l);
        }
        check_bounds(sa, sb, "draw", n);
        cases += 2;
    }
    std::printf("%d value cases\n", cases);
    std::printf(fails ? "%d checks FAILED\n" : "all checks passed\n", fails);
    return fails ? 1 : 0;
}
