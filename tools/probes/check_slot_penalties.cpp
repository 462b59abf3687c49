// The per-instance slack penalties of the host tables (ihm2_amd/csrc/qp_tables.hpp: find_penalty_mismatch, table_images) walked on the
// CPU.  Each argument is a problem file (tests/test_slot_penalties.py writes them; problem_file.hpp
// reads them).  Per problem, for B = 5 instances with penalties drawn inside the shared pattern (one of them with z = 0 on every side):
//   * instance b's block of the scattered table equals, entry for entry, zw / Zw of lay_out_slots on rows that hold b's penalties -- and
//     that table's kc, lb, ub are the shared table's (the layout depends on which sides are soft, not on the values);
//   * the (stage, side) copies equal those rows' sz / sZ and the a_lat pairs their alat_sz / alat_sZ;
//   * with one pair of arguments NULL those rows keep the shared penalties; an all-hard table is scattered onto itself;
//   * each half of each image sits at the offset the kernels use (`entries` in the slot images, NS*NC in the stage images), the bounds
//     halves hold the shared bounds, and with B = 1 and nothing per instance the images are the shared table and rows themselves;
//   * the pattern check refuses a flipped soft flag (both ways), z < 0, z = Z = 0 and a NaN, with the instance, stage and side.
// Per problem one line: name fit per_lane nsoft soft_slots.  Exit status 1 if any check failed.
// Build: g++ -std=c++17 -I ihm2_amd/csrc tools/probes/check_slot_penalties.cpp   (also with -fsanitize=address,undefined)
#include "problem_file.hpp"
#include "qp_catalogue.hpp"

using namespace ihm2;

static int fails = 0;
static std::string problem;
#define CHECK(c, ...) do { if (!(c)) { fails++; std::printf("FAIL %s %s:%d %s  ", problem.c_str(), __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static uint64_t lcg_state = 2463534242ull;
static double draw() { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg_state >> 11) / 9007199254740992.0; }

static bool same_bits(const double *a, const double *b, size_t n) { return n == 0 || std::memcmp(a, b, n * sizeof(double)) == 0; }

static const int B = 5;

struct Drawn { std::vector<double> iz, iZ, az, aZ; };

// penalties of B instances inside the pattern of `rows`; instance 2 has z = 0 wherever Z > 0
static Drawn draw_penalties(const ConstraintRows &rows)
{
    const size_t per = (size_t)rows.NS * NLAM;
    Drawn d;
    d.iz.assign(B * per, 0.0); d.iZ.assign(B * per, -1.0); d.az.assign(B * 2, 0.0); d.aZ.assign(B * 2, -1.0);
    for (int b = 0; b < B; b++) {
        for (size_t i = 0; i < per; i++) {
            if (!(rows.sZ[i] >= 0.0)) { d.iz[b * per + i] = 7.0 * draw(); continue; }     // a hard side: z is not read, Z stays hard
            d.iZ[b * per + i] = 1.0 + 500.0 * draw();
            d.iz[b * per + i] = (b == 2) ? 0.0 : 300.0 * draw();
        }
        for (int m = 0; m < 2; m++) {
            if (!(rows.alat_sZ[m] >= 0.0)) continue;
            d.aZ[b * 2 + m] = 1.0 + 500.0 * draw();
            d.az[b * 2 + m] = (b == 2) ? 0.0 : 300.0 * draw();
        }
    }
    return d;
}

static ConstraintRows rows_with(const ConstraintRows &rows, const Drawn &d, int b, bool stage, bool alat)
{
    ConstraintRows r = rows;
    const size_t per = (size_t)rows.NS * NLAM;
    if (stage) {
        r.sz.assign(d.iz.begin() + b * per, d.iz.begin() + (b + 1) * per);
        r.sZ.assign(d.iZ.begin() + b * per, d.iZ.begin() + (b + 1) * per);
    }
    if (alat)
        for (int m = 0; m < 2; m++) { r.alat_sz[m] = d.az[b * 2 + m]; r.alat_sZ[m] = d.aZ[b * 2 + m]; }
    return r;
}

static void check_scatter(const ConstraintRows &rows, const SlotTable &t, const std::vector<std::pair<int, int>> &limits, const Drawn &d,
                          bool stage, bool alat)
{
    const double *iz = stage ? d.iz.data() : nullptr, *iZ = stage ? d.iZ.data() : nullptr;
    const double *az = alat ? d.az.data() : nullptr, *aZ = alat ? d.aZ.data() : nullptr;
    const size_t n = t.entries(), per = (size_t)rows.NS * NLAM, nb = (size_t)rows.NS * NC;
    const TableImages m = table_images(t, rows, B, nullptr, nullptr, iz, iZ, az, aZ);
    CHECK(m.entries == n && m.stage_rows == nb, "%zu %zu", m.entries, m.stage_rows);
    CHECK(m.slot_lo.size() == B * 2 * n && m.slot_up.size() == B * 2 * n, "%zu", m.slot_lo.size());
    CHECK(m.stage_lo.size() == B * (nb + per) && m.stage_up.size() == B * (nb + per) && m.alat_z.size() == (size_t)B * 2 && m.alat_Z.size() == (size_t)B * 2, "%zu", m.stage_lo.size());
    if (fails) return;
    for (int b = 0; b < B; b++) {
        // instance b's blocks, the halves where the kernels look for them: zw / Zw `entries` doubles behind lb / ub, z / Z NS*NC behind the rows' bounds
        const double *slb = m.slot_lo.data() + b * 2 * n, *sub = m.slot_up.data() + b * 2 * n, *szw = slb + n, *sZw = sub + n;
        const double *stl = m.stage_lo.data() + b * (nb + per), *stu = m.stage_up.data() + b * (nb + per), *stz = stl + nb, *stZ = stu + nb;
        const ConstraintRows rb = rows_with(rows, d, b, stage, alat);
        const SlotTable tb = lay_out_slots(rb, limits);
        CHECK(tb.fit && tb.per_lane == t.per_lane && tb.nsoft == t.nsoft && tb.total == t.total && tb.m_act == t.m_act, "instance %d", b);
        CHECK(tb.kc == t.kc && tb.lb.size() == n && same_bits(tb.lb.data(), t.lb.data(), n) && same_bits(tb.ub.data(), t.ub.data(), n), "instance %d: the layout moved", b);
        if (tb.entries() != n) continue;
        for (size_t e = 0; e < n; e++) {
            CHECK(same_bits(&szw[e], &tb.zw[e], 1), "instance %d entry %zu: zw %g, laid out %g", b, e, szw[e], tb.zw[e]);
            CHECK(same_bits(&sZw[e], &tb.Zw[e], 1), "instance %d entry %zu: Zw %g, laid out %g", b, e, sZw[e], tb.Zw[e]);
            if (fails > 20) return;
        }
        CHECK(same_bits(stz, rb.sz.data(), per) && same_bits(stZ, rb.sZ.data(), per), "instance %d: stage copies", b);
        CHECK(same_bits(m.alat_z.data() + b * 2, rb.alat_sz, 2) && same_bits(m.alat_Z.data() + b * 2, rb.alat_sZ, 2), "instance %d: a_lat pairs", b);
        // no per-instance bounds: the bounds halves are the shared table's and the shared rows'
        CHECK(same_bits(slb, t.lb.data(), n) && same_bits(sub, t.ub.data(), n), "instance %d: slot bounds", b);
        CHECK(same_bits(stl, rows.lb.data(), nb) && same_bits(stu, rows.ub.data(), nb), "instance %d: stage bounds", b);
    }
}

// B = 1 and nothing per instance: the images are the batch-shared tables, each half where the kernels read it
static void check_shared_identity(const ConstraintRows &rows, const SlotTable &t)
{
    const size_t n = t.entries(), per = (size_t)rows.NS * NLAM, nb = (size_t)rows.NS * NC;
    const TableImages m = table_images(t, rows, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    CHECK(m.entries == n && m.stage_rows == nb && m.slot_lo.size() == 2 * n && m.slot_up.size() == 2 * n && m.stage_lo.size() == nb + per && m.stage_up.size() == nb + per, "sizes");
    if (fails) return;
    CHECK(same_bits(m.slot_lo.data(), t.lb.data(), n) && same_bits(m.slot_lo.data() + n, t.zw.data(), n), "slot_lo is not lb | zw");
    CHECK(same_bits(m.slot_up.data(), t.ub.data(), n) && same_bits(m.slot_up.data() + n, t.Zw.data(), n), "slot_up is not ub | Zw");
    CHECK(same_bits(m.stage_lo.data(), rows.lb.data(), nb) && same_bits(m.stage_lo.data() + nb, rows.sz.data(), per), "stage_lo is not lb | z");
    CHECK(same_bits(m.stage_up.data(), rows.ub.data(), nb) && same_bits(m.stage_up.data() + nb, rows.sZ.data(), per), "stage_up is not ub | Z");
    CHECK(same_bits(m.alat_z.data(), rows.alat_sz, 2) && same_bits(m.alat_Z.data(), rows.alat_sZ, 2), "a_lat pair");
}

static void expect(const ConstraintRows &rows, const Drawn &d, PenaltyMismatch::Kind kind, int b, int k, int side, const char *what)
{
    const PenaltyMismatch m = find_penalty_mismatch(rows, B, d.iz.data(), d.iZ.data(), d.az.data(), d.aZ.data());
    CHECK(m.kind == kind && m.b == b && m.k == k && m.side == side, "%s: kind %d at (%d, %d, %d), expected %d at (%d, %d, %d)", what, (int)m.kind, m.b, m.k,
          m.side, (int)kind, b, k, side);
}

static void check_refusals(const ConstraintRows &rows, const Drawn &good)
{
    using P = PenaltyMismatch;
    const size_t per = (size_t)rows.NS * NLAM;
    CHECK(!find_penalty_mismatch(rows, B, good.iz.data(), good.iZ.data(), good.az.data(), good.aZ.data()).found(), "the drawn penalties are refused");
    CHECK(!find_penalty_mismatch(rows, B, nullptr, nullptr, nullptr, nullptr).found(), "nothing given is refused");
    // the last soft and the last hard (stage, side) of the rows 0..13: in instance 3 every earlier entry is good
    int soft_i = -1, hard_i = -1;
    for (size_t i = 0; i < per; i++) (rows.sZ[i] >= 0.0 ? soft_i : hard_i) = (int)i;
    const int b = 3;
    if (soft_i >= 0) {
        const int k = soft_i / NLAM, side = soft_i % NLAM;
        Drawn d = good; d.iZ[b * per + soft_i] = -1.0;
        expect(rows, d, P::FLAG, b, k, side, "soft side made hard");
        d = good; d.iz[b * per + soft_i] = -1e-3;
        expect(rows, d, P::NEGATIVE, b, k, side, "z < 0");
        d = good; d.iz[b * per + soft_i] = NAN;
        expect(rows, d, P::NOT_A_NUMBER, b, k, side, "z NaN");
        d = good; d.iZ[b * per + soft_i] = NAN;
        expect(rows, d, P::NOT_A_NUMBER, b, k, side, "Z NaN");
        d = good; d.iz[b * per + soft_i] = 0.0; d.iZ[b * per + soft_i] = 0.0;
        expect(rows, d, P::NO_PENALTY, b, k, side, "z = Z = 0");
    }
    if (hard_i >= 0) {
        const int k = hard_i / NLAM, side = hard_i % NLAM;
        Drawn d = good; d.iZ[b * per + hard_i] = 10.0;
        expect(rows, d, P::FLAG, b, k, side, "hard side made soft");
        d = good; d.iz[b * per + hard_i] = NAN;
        expect(rows, d, P::NOT_A_NUMBER, b, k, side, "NaN on a hard side");
    }
    for (int m = 0; m < 2; m++) {
        Drawn d = good;
        d.aZ[b * 2 + m] = (rows.alat_sZ[m] >= 0.0) ? -1.0 : 10.0;
        expect(rows, d, P::FLAG, b, 0, NLAM + m, "a_lat flag");
        if (rows.alat_sZ[m] >= 0.0) {
            d = good; d.az[b * 2 + m] = -2.0;
            expect(rows, d, P::NEGATIVE, b, 0, NLAM + m, "a_lat z < 0");
        }
        d = good; d.az[b * 2 + m] = NAN;
        expect(rows, d, P::NOT_A_NUMBER, b, 0, NLAM + m, "a_lat NaN");
    }
}

int main(int argc, char **argv)
{
    for (int i = 1; i < argc; i++) {
        Problem p;
        if (!read_problem(argv[i], &p)) { std::printf("cannot read %s\n", argv[i]); return 2; }
        problem = p.name;
        const ConstraintRows rows = rows_of(p);
        const auto limits = slot_limits(p.alat ? 2 : p.path ? 1 : 0);
        const SlotTable t = lay_out_slots(rows, limits);
        int soft_slots = 0;
        for (size_t e = 0; e < t.entries(); e++) soft_slots += t.kc[e] >= 0 && t.Zw[e] >= 0.0;
        std::printf("%s %d %d %d %d\n", p.name.c_str(), (int)t.fit, t.per_lane, t.nsoft, soft_slots);
        CHECK(t.fit, "the layout fits no instantiation");
        if (!t.fit) continue;
        const Drawn d = draw_penalties(rows);
        check_scatter(rows, t, limits, d, true, true);
        check_scatter(rows, t, limits, d, true, false);
        check_scatter(rows, t, limits, d, false, true);
        check_scatter(rows, t, limits, d, false, false);
        check_shared_identity(rows, t);
        if (soft_slots == 0) {      // an all-hard table: the scatter is a no-op, whatever the instances hold
            const size_t n = t.entries();
            const TableImages m = table_images(t, rows, B, nullptr, nullptr, d.iz.data(), d.iZ.data(), d.az.data(), d.aZ.data());
            for (int b = 0; b < B; b++)
                CHECK(same_bits(m.slot_lo.data() + b * 2 * n + n, t.zw.data(), n) && same_bits(m.slot_up.data() + b * 2 * n + n, t.Zw.data(), n), "instance %d", b);
        }
        check_refusals(rows, d);
    }
    std::printf(fails ? "slot penalties: %d checks FAILED\n" : "slot penalties: all checks passed\n", fails);
    return fails ? 1 : 0;
}
