// The tables the host builds for the interior-point QP (ihm2_amd/csrc/qp_tables.hpp, qp_catalogue.hpp) walked on the CPU.  Each argument
// is a problem file (tests/test_slot_table.py writes them; problem_file.hpp reads them; C, D and the weights' flag are ignored here).
// The rows go through the functions api.hip calls, in the order of its setters; the table is then checked against what the kernels
// take from it unchecked (the list at the top of qp_tables.hpp), the device images (table_images) against values drawn inside the shared pattern,
// and the weight tables against the closed form of V'WV.  Per problem one line: name fit per_lane nsoft total m_act digest (FNV-1a over
// the bytes of kc, lb, ub, zw, Zw and the 256-lane kc, lb, ub).  Exit status 1 if any check failed.
// Build: g++ -std=c++17 -I ihm2_amd/csrc tools/probes/check_slot_table.cpp   (also with -fsanitize=address,undefined)
#include <cinttypes>
#include <map>

#include "problem_file.hpp"
#include "qp_catalogue.hpp"

using namespace ihm2;

static int fails = 0;
static std::string problem;
#define CHECK(c, ...) do { if (!(c)) { fails++; std::printf("FAIL %s %s:%d %s  ", problem.c_str(), __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static const double INF = INFINITY;

// ---- the rows stated once more, from the problem itself: row c = 0..14 of stage k with its sides and penalties ----
struct Side { bool finite, soft; double v, z, Z; };
struct Want { Side lo, up; };
static double absent_if_huge(double v, double absent) { return (v > -1e20 && v < 1e20) ? v : absent; }
static Want want_row(const Problem &p, int k, int c)
{
    const int N = p.N;
    double lb = -INF, ub = INF, zl = 0, Zl = -1, zu = 0, Zu = -1;
    if (c < 8 && k >= 1) { lb = p.lbx[k * 8 + c]; ub = p.ubx[k * 8 + c]; }
    if (c >= 8 && c < 10 && k < N) { lb = p.lbu[k * 2 + c - 8]; ub = p.ubu[k * 2 + c - 8]; }
    if (c >= 10 && c < 12 && k < N) { lb = p.lg[k * 2 + c - 10]; ub = p.ug[k * 2 + c - 10]; }
    if (c >= 12 && c < 14 && p.path && k >= 1) { lb = p.lh[c - 12]; ub = p.uh[c - 12]; }
    if (c < 14 && p.soft) { zl = p.soft_z[k * 28 + c]; Zl = p.soft_Z[k * 28 + c]; zu = p.soft_z[k * 28 + 14 + c]; Zu = p.soft_Z[k * 28 + 14 + c]; }
    if (c == 14 && p.alat && k >= 1 && k < N) { lb = p.alat_lb; ub = p.alat_ub; zl = p.alat_z[0]; Zl = p.alat_Z[0]; zu = p.alat_z[1]; Zu = p.alat_Z[1]; }
    lb = absent_if_huge(lb, -INF); ub = absent_if_huge(ub, INF);
    Want w;
    w.lo = {lb > -INF, lb > -INF && Zl >= 0, lb, zl, Zl};
    w.up = {ub < INF, ub < INF && Zu >= 0, ub, zu, Zu};
    return w;
}

static bool is_padding(const SlotTable &t, size_t e) { return t.kc[e] == -1 && t.lb[e] == -INF && t.ub[e] == INF && t.zw[e] == 0.0 && t.Zw[e] == -1.0; }
static bool one_sided(const SlotTable &t, size_t e) { return t.kc[e] >= 0 && ((t.lb[e] > -INF) != (t.ub[e] < INF)); }

static uint64_t fnv1a(uint64_t h, const void *data, size_t bytes)
{
    const unsigned char *p = (const unsigned char *)data;
    for (size_t i = 0; i < bytes; i++) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}
template <typename T>
static uint64_t fnv1a(uint64_t h, const std::vector<T> &v) { return fnv1a(h, v.data(), v.size() * sizeof(T)); }

// a generator of the probe's own (values only need to differ from the shared ones)
static uint64_t lcg_state = 88172645463325252ull;
static double draw() { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg_state >> 11) / 9007199254740992.0; }

static void check_table(const Problem &p, const ConstraintRows &rows, const SlotTable &t, const std::vector<std::pair<int, int>> &limits)
{
    const int NS = p.N + 1;
    int finite_sides = 0, soft_sides = 0;
    for (int k = 0; k < NS; k++)
        for (int c = 0; c < 15; c++) {
            const Want w = want_row(p, k, c);
            finite_sides += (int)w.lo.finite + (int)w.up.finite; soft_sides += (int)w.lo.soft + (int)w.up.soft;
        }
    // ---- the chosen instantiation ----
    bool first = true;
    for (const auto &lim : limits) {
        if (t.fit && lim.first == t.nsoft) break;
        first = first && !lay_out_slots(rows, {lim}).fit;
    }
    CHECK(first, "an earlier instantiation of the catalogue takes the rows");
    if (!t.fit) {
        CHECK(t.kc.empty() && t.lb.empty() && t.ub.empty() && t.zw.empty() && t.Zw.empty() && t.kc_blk.empty() && t.lb_blk.empty() && t.ub_blk.empty() &&
              t.per_lane == 0 && t.per_blk == 0 && t.total == 0, "a table that does not fit is empty");
        return;
    }
    const int S = t.nsoft;
    int NSL = -1;
    for (const auto &lim : limits) if (lim.first == S) NSL = lim.second;
    CHECK((S == 0) == (soft_sides == 0), "S %d with %d soft sides", S, soft_sides);
    CHECK(NSL >= 0 && t.per_lane <= NSL && 64 * t.per_lane <= MAX_SLOTS, "per_lane %d, NSLOT %d", t.per_lane, NSL);
    const size_t n = (size_t)64 * t.per_lane;
    CHECK(t.kc.size() == n && t.lb.size() == n && t.ub.size() == n && t.zw.size() == n && t.Zw.size() == n, "array sizes");
    if (t.kc.size() != n || t.lb.size() != n || t.ub.size() != n || t.zw.size() != n || t.Zw.size() != n) return;
    // ---- counts ----
    int total = 0;
    std::map<int, std::vector<size_t>> where;       // kc -> its entries
    for (size_t e = 0; e < n; e++) {
        if (t.kc[e] >= 0) { total++; where[t.kc[e]].push_back(e); }
        else CHECK(is_padding(t, e), "entry %zu: kc %d is neither a row nor padding", e, (int)t.kc[e]);
    }
    CHECK(t.total == total, "total %d, counted %d", t.total, total);
    CHECK(t.m_act == finite_sides + soft_sides, "m_act %d, %d finite + %d soft sides", t.m_act, finite_sides, soft_sides);
    // ---- row coverage ----
    size_t covered = 0;
    for (int k = 0; k < NS; k++)
        for (int c = 0; c < 15; c++) {
            const Want w = want_row(p, k, c);
            const auto it = where.find(k * 16 + c);
            if (!w.lo.finite && !w.up.finite) { CHECK(it == where.end(), "stage %d row %d has no finite side but an entry", k, c); continue; }
            CHECK(it != where.end(), "stage %d row %d is missing", k, c);
            if (it == where.end()) continue;
            const std::vector<size_t> &es = it->second;
            covered += es.size();
            if (!w.lo.soft && !w.up.soft) {
                CHECK(es.size() == 1 && t.lb[es[0]] == w.lo.v && t.ub[es[0]] == w.up.v && t.zw[es[0]] == 0.0 && t.Zw[es[0]] == -1.0, "hard row, stage %d row %d", k, c);
                continue;
            }
            CHECK(es.size() == (size_t)w.lo.finite + (size_t)w.up.finite, "split row, stage %d row %d: %zu entries", k, c, es.size());
            int lows = 0, ups = 0;
            for (size_t e : es) {
                CHECK(e % 64 == es[0] % 64, "split row, stage %d row %d: halves in the lanes %zu and %zu", k, c, es[0] % 64, e % 64);
                CHECK(one_sided(t, e), "split row, stage %d row %d: entry %zu is not one-sided", k, c, e);
                const bool lower = t.lb[e] > -INF;
                const Side &s = lower ? w.lo : w.up;
                (lower ? lows : ups)++;
                CHECK(s.finite && (lower ? t.lb[e] : t.ub[e]) == s.v, "split row, stage %d row %d: bound of the %s half", k, c, lower ? "lower" : "upper");
                CHECK(t.zw[e] == (s.soft ? s.z : 0.0) && t.Zw[e] == (s.soft ? s.Z : -1.0), "split row, stage %d row %d: penalties of the %s half", k, c, lower ? "lower" : "upper");
            }
            CHECK(lows == (int)w.lo.finite && ups == (int)w.up.finite, "split row, stage %d row %d: %d lower and %d upper halves", k, c, lows, ups);
        }
    CHECK(covered == (size_t)total, "%zu entries belong to rows, %d are not padding", covered, total);
    // ---- per-lane layout ----
    int load_min = 1 << 30, load_max = 0;
    for (int l = 0; l < 64; l++) {
        int load = 0;
        bool hard_seen = false;
        for (int r = 0; r < t.per_lane; r++) {
            const size_t e = l + 64 * (size_t)r;
            load += t.kc[e] >= 0;
            const bool soft = t.Zw[e] >= 0.0;
            if (soft) CHECK(r < S && one_sided(t, e), "lane %d entry %d: a soft entry behind the leading %d, or two-sided", l, r, S);
            if (r < S) {
                CHECK(one_sided(t, e) || is_padding(t, e), "lane %d entry %d of the leading %d is two-sided", l, r, S);
                CHECK(!(soft && hard_seen), "lane %d entry %d: a soft entry behind a hard one among the leading %d", l, r, S);
                hard_seen = hard_seen || !soft;
            }
        }
        load_min = std::min(load_min, load); load_max = std::max(load_max, load);
    }
    if (S == 0) CHECK(load_max - load_min <= 1, "all-hard table: lane loads %d .. %d", load_min, load_max);
    // ---- the 256-lane table ----
    const bool blk = S == 0 && total > 0 && total <= 1024;
    CHECK((t.per_blk > 0) == blk, "per_blk %d", t.per_blk);
    if (blk) {
        const size_t nb = (size_t)t.per_blk * 256;
        CHECK(t.per_blk == (int)((n + 255) / 256) && t.kc_blk.size() == nb && t.lb_blk.size() == nb && t.ub_blk.size() == nb, "per_blk %d for %zu entries", t.per_blk, n);
        if (t.kc_blk.size() != nb || t.lb_blk.size() != nb || t.ub_blk.size() != nb) return;
        for (size_t e = 0; e < nb; e++) {
            const bool same = e < n ? (t.kc_blk[e] == t.kc[e] && t.lb_blk[e] == t.lb[e] && t.ub_blk[e] == t.ub[e]) : (t.kc_blk[e] == -1 && t.lb_blk[e] == -INF && t.ub_blk[e] == INF);
            CHECK(same, "entry %zu of the 256-lane table", e);
        }
    } else {
        CHECK(t.kc_blk.empty() && t.lb_blk.empty() && t.ub_blk.empty(), "no 256-lane table");
    }
}

static void check_scatter(const Problem &p, const ConstraintRows &rows, const SlotTable &t)
{
    const int B = 3, N = p.N, NS = N + 1;
    // per-instance values inside the shared pattern: every finite bound moved a little, absent sides written in the three ways
    std::vector<double> il((size_t)B * NS * 12), iu(il.size());
    for (int b = 0; b < B; b++) {
        std::vector<double> v[6] = {p.lbx, p.ubx, p.lbu, p.ubu, p.lg, p.ug};
        for (auto &a : v)
            for (double &x : a) x = (x > -1e20 && x < 1e20) ? x + draw() : (x < 0 ? -1.0 : 1.0) * (b == 0 ? 1e20 : b == 1 ? 1e25 : INF);
        box_rows(N, v[0].data(), v[1].data(), v[2].data(), v[3].data(), v[4].data(), v[5].data(), &il[(size_t)b * NS * 12], &iu[(size_t)b * NS * 12], 12);
    }
    CHECK(!find_pattern_mismatch(rows, B, il.data(), iu.data()).found, "values inside the pattern are refused");
    const TableImages m = table_images(t, rows, B, il.data(), iu.data(), nullptr, nullptr, nullptr, nullptr);
    const size_t n = t.entries(), nb = (size_t)NS * NC, np = (size_t)NS * NLAM;
    CHECK(m.entries == n && m.stage_rows == nb && m.slot_lo.size() == B * 2 * n && m.slot_up.size() == B * 2 * n && m.stage_lo.size() == B * (nb + np) &&
          m.stage_up.size() == m.stage_lo.size(), "sizes");
    if (m.slot_lo.size() != B * 2 * n || m.slot_up.size() != B * 2 * n || m.stage_lo.size() != B * (nb + np) || m.stage_up.size() != B * (nb + np)) return;
    int moved = 0, wanted = 0;
    for (int b = 0; b < B; b++) {
        // instance b's halves, at the offsets the kernels use: the penalties `entries` behind the slot bounds, NS*NC behind the rows' bounds
        const double *slb = m.slot_lo.data() + (size_t)b * 2 * n, *sub = m.slot_up.data() + (size_t)b * 2 * n;
        const double *stl = m.stage_lo.data() + (size_t)b * (nb + np), *stu = m.stage_up.data() + (size_t)b * (nb + np);
        // no per-instance penalties: the second halves are the shared table's zw / Zw and the shared rows' sz / sZ
        CHECK(std::equal(t.zw.begin(), t.zw.end(), slb + n) && std::equal(t.Zw.begin(), t.Zw.end(), sub + n), "instance %d: slot penalties", b);
        CHECK(std::equal(rows.sz.begin(), rows.sz.end(), stl + nb) && std::equal(rows.sZ.begin(), rows.sZ.end(), stu + nb), "instance %d: stage penalties", b);
        for (size_t e = 0; e < n; e++) {
            const int kc = t.kc[e], k = kc >> 4, c = kc & 15;
            const bool mine = kc >= 0 && c < 12;
            const size_t i = mine ? ((size_t)b * NS + k) * 12 + c : 0;
            const double lo = (mine && t.lb[e] > -INF) ? il[i] : t.lb[e], up = (mine && t.ub[e] < INF) ? iu[i] : t.ub[e];
            CHECK(slb[e] == lo && sub[e] == up, "instance %d entry %zu (stage %d row %d)", b, e, k, c);
            moved += (int)(slb[e] != t.lb[e]) + (int)(sub[e] != t.ub[e]);
        }
        for (int k = 0; k < NS; k++)
            for (int c = 0; c < NC; c++) {
                const size_t i = ((size_t)b * NS + k) * 12 + c;
                CHECK(stl[k * NC + c] == (c < 12 ? il[i] : rows.lb[k * NC + c]) && stu[k * NC + c] == (c < 12 ? iu[i] : rows.ub[k * NC + c]), "instance %d stage %d row %d of the (NS,NC) bounds", b, k, c);
                if (c < 12) wanted += (int)std::isfinite(il[i]) + (int)std::isfinite(iu[i]);
            }
    }
    {       // B = 1, nothing per instance: the images are the batch-shared table and rows
        const TableImages s1 = table_images(t, rows, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        CHECK(s1.slot_lo.size() == 2 * n && s1.slot_up.size() == 2 * n && s1.stage_lo.size() == nb + np && s1.stage_up.size() == nb + np, "sizes of the shared images");
        if (s1.slot_lo.size() != 2 * n || s1.slot_up.size() != 2 * n || s1.stage_lo.size() != nb + np || s1.stage_up.size() != nb + np) return;
        CHECK(std::equal(t.lb.begin(), t.lb.end(), s1.slot_lo.begin()) && std::equal(t.zw.begin(), t.zw.end(), s1.slot_lo.begin() + n), "shared slot_lo is not lb | zw");
        CHECK(std::equal(t.ub.begin(), t.ub.end(), s1.slot_up.begin()) && std::equal(t.Zw.begin(), t.Zw.end(), s1.slot_up.begin() + n), "shared slot_up is not ub | Zw");
        CHECK(std::equal(rows.lb.begin(), rows.lb.end(), s1.stage_lo.begin()) && std::equal(rows.sz.begin(), rows.sz.end(), s1.stage_lo.begin() + nb), "shared stage_lo is not lb | z");
        CHECK(std::equal(rows.ub.begin(), rows.ub.end(), s1.stage_up.begin()) && std::equal(rows.sZ.begin(), rows.sZ.end(), s1.stage_up.begin() + nb), "shared stage_up is not ub | Z");
    }
    CHECK(moved == wanted, "%d sides of the table took an instance's value, the instances have %d finite sides", moved, wanted);
    // one side outside the pattern
    const int b = B - 1, k = NS / 2, c = 9;
    const size_t i = ((size_t)b * NS + k) * 12 + c;
    const bool shared = std::isfinite(rows.lb[k * NC + c]);
    il[i] = shared ? -INF : 0.0;
    const PatternMismatch mm = find_pattern_mismatch(rows, B, il.data(), iu.data());
    CHECK(mm.found && mm.b == b && mm.k == k && mm.c == c && mm.lower == !shared && mm.shared_lower == shared && mm.upper == mm.shared_upper,
          "mismatch reported at instance %d stage %d row %d", mm.b, mm.k, mm.c);
}

// Hs = c V'WV and Gy = c V'W for y = V z = [x; u; x[6:8] - u]: column i of V has a 1 in row i, the columns 6, 7 another 1 in the rows 10, 11
// and the columns 8, 9 a -1 there -- summed over those entries only
static void check_weights()
{
    problem = "weights";
    const double cs = 0.05;
    double W[144], We[64];
    for (int i = 0; i < 12; i++) for (int j = 0; j <= i; j++) W[i * 12 + j] = W[j * 12 + i] = draw() - 0.5 + (i == j ? 12.0 : 0.0);
    for (int i = 0; i < 8; i++) for (int j = 0; j <= i; j++) We[i * 8 + j] = We[j * 8 + i] = draw() - 0.5 + (i == j ? 8.0 : 0.0);
    double H[100], G[120];
    stage_weight_tables(W, cs, H, G);
    struct Term { int row; double a; };
    auto column = [](int i) { return i < 6 ? std::vector<Term>{{i, 1.0}} : i < 8 ? std::vector<Term>{{i, 1.0}, {i + 4, 1.0}} : std::vector<Term>{{i, 1.0}, {i + 2, -1.0}}; };
    double worst = 0.0;
    for (int i = 0; i < 10; i++) {
        double vtw[12];
        for (int j = 0; j < 12; j++) {
            vtw[j] = 0.0;
            for (const Term &t : column(i)) vtw[j] += t.a * W[t.row * 12 + j];
            worst = std::max(worst, std::fabs(G[i * 12 + j] - cs * vtw[j]));
        }
        for (int j = 0; j < 10; j++) {
            double acc = 0.0;
            for (const Term &t : column(j)) acc += vtw[t.row] * t.a;
            worst = std::max(worst, std::fabs(H[i * 10 + j] - cs * acc));
        }
    }
    CHECK(worst == 0.0, "stage tables against the closed form: %g", worst);      // (the same sums without the selector's zeros)
    CHECK(symmetric10(H), "V'WV of a symmetric W");
    H[3 * 10 + 7] += 1e-6;
    CHECK(!symmetric10(H), "an asymmetric Hessian passes");
    double HN[100] = {0}, GN[120] = {0};
    terminal_weight_tables(We, HN, GN);
    for (int i = 0; i < 10; i++) {
        for (int j = 0; j < 10; j++) CHECK(HN[i * 10 + j] == (i < 8 && j < 8 ? We[i * 8 + j] : i == j ? 1.0 : 0.0), "terminal Hessian [%d][%d]", i, j);
        for (int j = 0; j < 12; j++) CHECK(GN[i * 12 + j] == (i < 8 && j < 8 ? We[i * 8 + j] : 0.0), "terminal gradient map [%d][%d]", i, j);
    }
    // uniformity against a direct comparison: equal stages, then one entry of one stage moved
    for (int N = 1; N <= 4; N++)
        for (int moved = -1; moved < N * 7; moved++) {
            std::vector<double> T((size_t)N * 7);
            for (int k = 0; k < N; k++) for (int i = 0; i < 7; i++) T[k * 7 + i] = 1.0 + i;
            if (moved >= 0) T[moved] += 1.0;
            bool same = true;
            for (int k = 1; k < N; k++) same = same && std::equal(T.begin(), T.begin() + 7, T.begin() + k * 7);
            CHECK(stages_equal(T.data(), N, 7) == same, "N %d, entry %d moved", N, moved);
        }
}

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        Problem p;
        problem = argv[a];
        if (!read_problem(argv[a], &p)) { fails++; std::printf("FAIL %s: not a problem file\n", argv[a]); continue; }
        problem = p.name;
        const ConstraintRows rows = rows_of(p);
        const auto limits = slot_limits(p.alat ? 2 : p.path ? 1 : 0);
        const SlotTable t = lay_out_slots(rows, limits);
        check_table(p, rows, t, limits);
        if (t.fit) check_scatter(p, rows, t);
        uint64_t h = 14695981039346656037ull;
        h = fnv1a(h, t.kc); h = fnv1a(h, t.lb); h = fnv1a(h, t.ub); h = fnv1a(h, t.zw); h = fnv1a(h, t.Zw);
        h = fnv1a(h, t.kc_blk); h = fnv1a(h, t.lb_blk); h = fnv1a(h, t.ub_blk);
        std::printf("%s %d %d %d %d %d %016" PRIx64 "\n", p.name.c_str(), (int)t.fit, t.per_lane, t.nsoft, t.total, t.m_act, h);
    }
    check_weights();
    if (fails) std::printf("%d checks failed\n", fails);
    else std::printf("slot tables: all checks passed\n");
    return fails != 0;
}
