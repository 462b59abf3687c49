// qp_tables.hpp -- the tables the host builds for the interior-point QP: the constraint rows as the setters leave them, the slot table the
// kernels read them from, the per-instance values scattered into its pattern, and the weight tables.  Plain C++17 without HIP and without
// the handle: api.hip calls these functions, and tools/probes/check_slot_table.cpp (tests/test_slot_table.py) walks them on any machine.
//
// What k_qp_wave, k_qp_block and k_steps take from the slot table WITHOUT checking it (kernels_qp.hip):
//   * entry lane + 64 r belongs to lane `lane`; both halves of a split row sit in one lane (they accumulate into the same LDS words
//     without atomics);
//   * a lane's first NSOFT entries are one-sided, its soft ones first (ONE_SIDED: the kernel keeps slack registers, and one side's
//     registers only, for those);
//   * padding is kc = -1 with infinite bounds;
//   * the 256-lane table is the 64-lane table entry for entry (the four-wave kernel's results are then the one-wave kernel's bit for bit);
//   * the order of the entries is the order of the slot sums, and with it every bit of the results.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "ihm2_dims.h"

namespace ihm2 {

// ---- rows ----

// a bound as the setters take it: |v| >= 1e20 is an absent side
inline double bound_or(double v, double absent) { return (std::fabs(v) < 1e20) ? v : absent; }

struct Bounds { double lb, ub; };
// Row c = 0..11 of stage k as given (state boxes lbx/ubx (N+1,8), input boxes lbu/ubu (N,2), general rows lg/ug (N,2)): stage 0 has no
// state box (x_0 is fixed), stage N neither input nor general rows.
inline Bounds box_row(int N, int k, int c, const double *lbx, const double *ubx, const double *lbu, const double *ubu, const double *lg, const double *ug)
{
    if (c < 8) return (k >= 1) ? Bounds{lbx[k * 8 + c], ubx[k * 8 + c]} : Bounds{-INFINITY, INFINITY};
    if (k >= N) return {-INFINITY, INFINITY};
    return (c < 10) ? Bounds{lbu[k * 2 + c - 8], ubu[k * 2 + c - 8]} : Bounds{lg[k * 2 + c - 10], ug[k * 2 + c - 10]};
}

// The rows 0..11 of the stages 0..N from those arrays into lb, ub (`stride` doubles per stage), +-inf where a side is absent: the
// batch-shared table (stride NC) and one instance's values (stride 12) alike.
inline void box_rows(int N, const double *lbx, const double *ubx, const double *lbu, const double *ubu, const double *lg, const double *ug,
                     double *lb, double *ub, int stride)
{
    for (int k = 0; k <= N; k++)
        for (int c = 0; c < 12; c++) {
            const Bounds r = box_row(N, k, c, lbx, ubx, lbu, ubu, lg, ug);
            lb[k * stride + c] = bound_or(r.lb, -INFINITY);
            ub[k * stride + c] = bound_or(r.ub, INFINITY);
        }
}

// The constraint rows the slot table is laid out from; the setters come one by one and in any order.
struct ConstraintRows {
    int NS = 0;
    std::vector<double> lb, ub;     // (NS,NC) per (stage, row), +-inf = absent
    std::vector<double> sz, sZ;     // (NS,NLAM) slack penalties per one-sided constraint: NC lower then NC upper; sZ < 0 = hard
    // the lateral-acceleration row of the kinematic constraint set (row 14 of the stages 1..N-1), kept beside the NC rows of the tables
    int alat_on = 0;
    double alat_lb = -INFINITY, alat_ub = INFINITY, alat_sz[2] = {0.0, 0.0}, alat_sZ[2] = {-1.0, -1.0};     // [2]: lower / upper side

    ConstraintRows() = default;
    explicit ConstraintRows(int ns) : NS(ns), lb(ns * NC, -INFINITY), ub(ns * NC, INFINITY), sz(ns * NLAM, 0.0), sZ(ns * NLAM, -1.0) {}

    // rows 0..11 (ihm2mpc_set_bounds); rows 12, 13 belong to set_track_rows
    void set_box_rows(const double *lbx, const double *ubx, const double *lbu, const double *ubu, const double *lg, const double *ug)
    {
        box_rows(NS - 1, lbx, ubx, lbu, ubu, lg, ug, lb.data(), ub.data(), NC);
    }
    // rows 12, 13 of the stages 1..N (ihm2mpc_set_path_constraints); x_0 is fixed: the rows of stage 0 are constants
    void set_track_rows(bool enable, const double *lh, const double *uh)
    {
        for (int k = 0; k < NS; k++)
            for (int i = 0; i < NH; i++) {
                const bool on = enable && k >= 1;
                lb[k * NC + 12 + i] = on ? bound_or(lh[i], -INFINITY) : -INFINITY;
                ub[k * NC + 12 + i] = on ? bound_or(uh[i], INFINITY) : INFINITY;
            }
    }
};

// ---- layout ----

struct SlotTable {
    bool fit = false;       // an instantiation takes the rows; false: everything below is empty
    int per_lane = 0;       // slots per lane
    int nsoft = 0;          // leading one-sided entries per lane: the NSOFT of the instantiation that takes the table (0: all-hard)
    int total = 0;          // entries that are not padding
    int m_act = 0;          // one-sided inequality pairs: finite sides + one per soft slack
    // entry lane + 64 r, 64 per_lane of each: stage * 16 + row (-1 = padding), raw bounds (+-inf = absent side; soft slots are one-sided),
    // slack cost zw s + 1/2 Zw s^2 of a soft slot (Zw < 0 = hard slot)
    std::vector<int32_t> kc;
    std::vector<double> lb, ub, zw, Zw;
    // the same rows over 256 lanes for the four-wave latency kernel (thread t of the block holds the entries t, t + 256, ...): entry e IS
    // entry e of the 64-lane table.  All-hard tables with 0 < total <= 1024 only, else per_blk = 0 and the arrays are empty.
    int per_blk = 0;
    std::vector<int32_t> kc_blk;
    std::vector<double> lb_blk, ub_blk;

    size_t entries() const { return kc.size(); }
};

namespace slot_detail {

struct Slot { int kc; double lb, ub, zw, Zw; };
const Slot PADDING = {-1, -INFINITY, INFINITY, 0.0, -1.0};

// a row with a finite side: fl, fu its finite sides, sl, su the soft ones among them
struct Row {
    int kc;
    double lb, ub, szl, sZl, szu, sZu;
    bool fl, fu, sl, su;
    bool soft() const { return sl || su; }
    bool two_sided() const { return fl && fu; }
    int nsoft() const { return (int)sl + (int)su; }
};

// the rows with a finite side, stage-major
inline std::vector<Row> finite_rows(const ConstraintRows &c)
{
    std::vector<Row> rows;
    for (int k = 0; k < c.NS; k++)
        for (int r = 0; r < NC + 1; r++) {
            const bool extra = r == NC;
            if (extra && !(c.alat_on && k >= 1 && k < c.NS - 1)) continue;
            Row row;
            row.kc = k * 16 + r;
            row.lb = extra ? c.alat_lb : c.lb[k * NC + r]; row.ub = extra ? c.alat_ub : c.ub[k * NC + r];
            row.fl = std::isfinite(row.lb); row.fu = std::isfinite(row.ub);
            if (!row.fl && !row.fu) continue;
            row.szl = extra ? c.alat_sz[0] : c.sz[k * NLAM + r]; row.sZl = extra ? c.alat_sZ[0] : c.sZ[k * NLAM + r];
            row.szu = extra ? c.alat_sz[1] : c.sz[k * NLAM + NC + r]; row.sZu = extra ? c.alat_sZ[1] : c.sZ[k * NLAM + NC + r];
            row.sl = row.fl && row.sZl >= 0.0; row.su = row.fu && row.sZu >= 0.0;
            rows.push_back(row);
        }
    return rows;
}

// What a lane holds while the rows are dealt out for an instantiation with S leading entries: its one-sided slots (which may lead) and its
// two-sided ones (which may not).
struct Lane {
    std::vector<Slot> ones, twos;
    int nsoft = 0;
    int size() const { return (int)(ones.size() + twos.size()); }
    int tail(int S) const { return (int)twos.size() + std::max(0, (int)ones.size() - S); }      // entries behind the first S
    // What the lane costs as the home of row r; the row goes to the cheapest lane, ties to the lowest.  A row with a soft side (dealt out
    // first): by soft sides, then by entries.  A hard row: by the entries behind the leading ones it would leave the lane with -- a
    // one-sided row is free while a leading entry is (all-hard tables, S = 0: by entries, which is round-robin).
    std::pair<int, int> cost(const Row &r, int S) const
    {
        if (r.soft()) return {nsoft, size()};
        const bool leads = S > 0 && !r.two_sided() && (int)ones.size() < S;
        return {0, tail(S) - (leads ? 1 : 0)};
    }
    void take(const Row &r, int S)
    {
        if (!r.soft()) {
            (S > 0 && !r.two_sided() ? ones : twos).push_back({r.kc, r.lb, r.ub, 0.0, -1.0});       // a hard one-sided row may lead
            return;
        }
        // a row with a soft side is split into its sides, the soft half in front of a hard half
        const Slot lo = {r.kc, r.lb, INFINITY, r.sl ? r.szl : 0.0, r.sl ? r.sZl : -1.0}, up = {r.kc, -INFINITY, r.ub, r.su ? r.szu : 0.0, r.su ? r.sZu : -1.0};
        if (r.sl) ones.push_back(lo);
        if (r.su) ones.push_back(up);
        if (r.fl && !r.sl) ones.push_back(lo);
        if (r.fu && !r.su) ones.push_back(up);
        nsoft += r.nsoft();
    }
    // the lane's entries in table order: S leading one-sided entries, its soft ones first (padding where it has fewer and something
    // follows), then the rest
    std::vector<Slot> entries(int S) const
    {
        std::vector<Slot> lead = ones;
        std::stable_partition(lead.begin(), lead.end(), [](const Slot &s) { return s.Zw >= 0.0; });
        std::vector<Slot> e(lead.begin(), lead.begin() + std::min(S, (int)lead.size()));
        if (tail(S) > 0) e.resize(S, PADDING);
        if ((int)lead.size() > S) e.insert(e.end(), lead.begin() + S, lead.end());
        e.insert(e.end(), twos.begin(), twos.end());
        return e;
    }
};

}  // namespace slot_detail

// The slot table of the rows for the first of `limits` that takes them: (NSOFT, the largest NSLOT that comes with it) of the per-step
// QP's instantiations for these rows, in catalogue order (qp_catalogue.hpp: slot_limits); NSOFT = 0 is for the all-hard table, NSOFT > 0
// for the rows with soft sides.  fit = false: none takes them.
inline SlotTable lay_out_slots(const ConstraintRows &c, const std::vector<std::pair<int, int>> &limits)
{
    using namespace slot_detail;
    const std::vector<Row> rows = finite_rows(c);
    SlotTable t;
    int soft_total = 0;
    for (const Row &r : rows) { soft_total += r.nsoft(); t.m_act += (int)r.fl + (int)r.fu + r.nsoft(); }
    for (const auto &lim : limits) {
        const int S = lim.first, NSL = lim.second;
        if ((S == 0) != (soft_total == 0)) continue;
        // two passes: the rows with a soft side first, then the hard rows
        Lane lanes[64];
        for (const bool soft : {true, false})
            for (const Row &r : rows) {
                if (r.soft() != soft) continue;
                Lane *best = &lanes[0];
                for (Lane &l : lanes)
                    if (l.cost(r, S) < best->cost(r, S)) best = &l;
                best->take(r, S);
            }
        int per_lane = 0, soft_max = 0;
        for (const Lane &l : lanes) { per_lane = std::max(per_lane, S + l.tail(S)); soft_max = std::max(soft_max, l.nsoft); }
        if (soft_max > S || per_lane > NSL) continue;
        // (a lane that has leading entries only is not padded up to S: the table may be shorter than S + the longest tail)
        per_lane = 0;
        std::vector<Slot> entries[64];
        for (int l = 0; l < 64; l++) { entries[l] = lanes[l].entries(S); per_lane = std::max(per_lane, (int)entries[l].size()); }
        if (per_lane * 64 > MAX_SLOTS) break;
        t.fit = true; t.per_lane = per_lane; t.nsoft = S;
        const size_t n = (size_t)per_lane * 64;
        t.kc.assign(n, PADDING.kc); t.lb.assign(n, PADDING.lb); t.ub.assign(n, PADDING.ub); t.zw.assign(n, PADDING.zw); t.Zw.assign(n, PADDING.Zw);
        for (int l = 0; l < 64; l++)
            for (size_t r = 0; r < entries[l].size(); r++) {
                const Slot &s = entries[l][r];
                const size_t e = l + 64 * r;
                t.kc[e] = s.kc; t.lb[e] = s.lb; t.ub[e] = s.ub; t.zw[e] = s.zw; t.Zw[e] = s.Zw;
                t.total += s.kc >= 0;
            }
        if (S == 0 && t.total > 0 && t.total <= 1024) {
            t.per_blk = ((int)n + 255) / 256;
            const size_t nb = (size_t)t.per_blk * 256;
            t.kc_blk = t.kc; t.lb_blk = t.lb; t.ub_blk = t.ub;
            t.kc_blk.resize(nb, PADDING.kc); t.lb_blk.resize(nb, PADDING.lb); t.ub_blk.resize(nb, PADDING.ub);
        }
        break;
    }
    if (!t.fit) t.m_act = 0;
    return t;
}

// ---- the full table ----
// What the kernels' full slot form (kernels_qp.hip: qp_wave_body, FULL) takes WITHOUT asking, in every slot loop of every iteration: the
// table is all-hard, holds no track or a_lat row, every lane owns exactly `nslot` entries (the instantiation's NSLOT) and none of the
// 64 nslot entries is padding, and both bounds of every entry are finite -- by the kernel's own test, |v| < 1e20.  The reference's rows
// are such a table at N = 40 (8 N = 320 = 64 x 5 two-sided rows) and at no other horizon.
inline bool full_bound(double v) { return std::fabs(v) < 1e20; }
inline bool slot_table_full(const SlotTable &t, int nslot)
{
    if (!t.fit || t.nsoft != 0 || t.per_lane != nslot || t.total != 64 * nslot || t.entries() != (size_t)64 * nslot) return false;
    for (size_t e = 0; e < t.entries(); e++) {
        const int kc = t.kc[e];
        if (kc < 0 || (kc & 15) >= 12 || t.Zw[e] >= 0.0) return false;
        if (!full_bound(t.lb[e]) || !full_bound(t.ub[e])) return false;
    }
    return true;
}
// ... and with per-instance bounds: those of every instance, read from the bounds half of the slot images (table_images below: (B, 2,
// entries) each).  A second line of defence: the setter refuses per-instance values whose finite sides differ from the shared table's
// (find_pattern_mismatch) before an image is built, so once slot_table_full holds no call of the library reaches this function with an
// infinite value -- only the CPU probe (tools/probes/check_full_table.cpp) does.  It stays because the kernel asks nothing, and the
// pattern check may change.
inline bool slot_bounds_full(const SlotTable &t, int B, const std::vector<double> &slot_lo, const std::vector<double> &slot_up)
{
    const size_t n = t.entries();
    if (slot_lo.size() != (size_t)B * 2 * n || slot_up.size() != (size_t)B * 2 * n) return false;
    for (size_t b = 0; b < (size_t)B; b++)
        for (size_t e = 0; e < n; e++)
            if (!full_bound(slot_lo[b * 2 * n + e]) || !full_bound(slot_up[b * 2 * n + e])) return false;
    return true;
}

// ---- per-instance bounds in the pattern of the batch-shared table ----
// il, iu (B,NS,12): the values of the rows 0..11 per instance, +-inf = absent (box_rows with stride 12).

// the first (instance, stage, row) whose finite sides differ from the shared rows', with the sides of both
struct PatternMismatch {
    bool found;
    int b, k, c;
    bool lower, upper, shared_lower, shared_upper;
};
inline PatternMismatch find_pattern_mismatch(const ConstraintRows &rows, int B, const double *il, const double *iu)
{
    const int NS = rows.NS;
    for (int b = 0; b < B; b++)
        for (int k = 0; k < NS; k++)
            for (int c = 0; c < 12; c++) {
                const size_t i = ((size_t)b * NS + k) * 12 + c;
                const bool lo = std::isfinite(il[i]), up = std::isfinite(iu[i]);
                const bool slo = std::isfinite(rows.lb[k * NC + c]), sup = std::isfinite(rows.ub[k * NC + c]);
                if (lo != slo || up != sup) return {true, b, k, c, lo, up, slo, sup};
            }
    return {false, 0, 0, 0, false, false, false, false};
}

// ---- per-instance slack penalties in the pattern of the batch-shared table ----
// iz, iZ (B,NS,NLAM): the penalties of the rows 0..13 per instance, the layout of ConstraintRows::sz / sZ; az, aZ (B,2): those of the
// a_lat row, lower / upper side.  Either pair may be nullptr: those rows keep the batch-shared penalties.

// the first (instance, stage, side) whose penalties the shared pattern does not take; side = 0..27 as in sz / sZ (NC lower, then NC
// upper sides), 28 / 29 = lower / upper side of the a_lat row (stage 0: the row's penalties do not depend on the stage)
struct PenaltyMismatch {
    enum Kind { NONE = 0, FLAG, NEGATIVE, NOT_A_NUMBER, NO_PENALTY } kind;
    int b, k, side;
    bool soft, shared_soft;
    bool found() const { return kind != NONE; }
};
namespace slot_detail {
// one side's (z, Z) against the shared Z of that side
inline PenaltyMismatch::Kind penalty_side(double z, double Z, double shared_Z)
{
    if (z != z || Z != Z) return PenaltyMismatch::NOT_A_NUMBER;
    if ((Z >= 0.0) != (shared_Z >= 0.0)) return PenaltyMismatch::FLAG;
    if (Z >= 0.0 && !(z >= 0.0)) return PenaltyMismatch::NEGATIVE;
    if (Z >= 0.0 && !(Z + z > 0.0)) return PenaltyMismatch::NO_PENALTY;
    return PenaltyMismatch::NONE;
}
}  // namespace slot_detail
// A side is soft (Z >= 0) for an instance exactly where the shared rows hold it soft (FLAG); z >= 0 on a soft side (NEGATIVE); no NaN
// anywhere (NOT_A_NUMBER); and, as ihm2mpc_set_soft refuses it for the shared table, no soft side with z = Z = 0, which has neither a
// linear nor a quadratic penalty (NO_PENALTY).  What an instance gives on a hard side is otherwise not read.
inline PenaltyMismatch find_penalty_mismatch(const ConstraintRows &rows, int B, const double *iz, const double *iZ, const double *az, const double *aZ)
{
    const int NS = rows.NS;
    for (int b = 0; b < B; b++) {
        if (iz && iZ)
            for (int k = 0; k < NS; k++)
                for (int i = 0; i < NLAM; i++) {
                    const size_t e = ((size_t)b * NS + k) * NLAM + i;
                    const PenaltyMismatch::Kind kind = slot_detail::penalty_side(iz[e], iZ[e], rows.sZ[k * NLAM + i]);
                    if (kind) return {kind, b, k, i, iZ[e] >= 0.0, rows.sZ[k * NLAM + i] >= 0.0};
                }
        if (az && aZ)
            for (int m = 0; m < 2; m++) {
                const PenaltyMismatch::Kind kind = slot_detail::penalty_side(az[b * 2 + m], aZ[b * 2 + m], rows.alat_sZ[m]);
                if (kind) return {kind, b, 0, NLAM + m, aZ[b * 2 + m] >= 0.0, rows.alat_sZ[m] >= 0.0};
            }
    }
    return {PenaltyMismatch::NONE, 0, 0, 0, false, false};
}

// ---- the device images ----
// The constraint tables as the kernels read them, for B instances (B = 1 with every per-instance array nullptr: the batch-shared tables).
// Each table is one pair of arrays with two halves per instance, so that one base per instance serves the bounds and the penalties:
//   slot_lo, slot_up    (B, 2, entries)             lb | zw and ub | Zw of the slot table; the second half starts at `entries`
//   stage_lo, stage_up  (B, NS*NC + NS*NLAM)        lb | z and ub | Z per (stage, row) and (stage, side): the SQP mode's line search and
//                                                   the cost; the second half starts at NS*NC
//   alat_z, alat_Z      (B, 2)                      the a_lat row's penalties, lower / upper side: the cost
// il, iu (B,NS,12); iz, iZ (B,NS,NLAM); az, aZ (B,2) as above; each pair may be nullptr: those rows hold the batch-shared values.
//   * bounds of a slot: the value of instance b where the shared entry has that side finite, in the rows 0..11; the track rows, the
//     a_lat row and the absent side of a split (soft) row's halves keep the shared value;
//   * penalties of a slot: the values of instance b on the soft slots -- a soft slot is one-sided, the side its finite bound -- and the
//     shared table's on the hard slots and the padding.  Instance b's block is then the zw, Zw of lay_out_slots on rows that hold b's
//     penalties: the layout depends on which sides are soft, not on the values;
//   * (stage, row) bounds: the rows 0..11 per instance, the track rows batch-shared; (stage, side) penalties and the a_lat pairs: the
//     instance's values as given.
struct TableImages {
    size_t entries = 0, stage_rows = 0;     // offsets of the second halves: SlotTable::entries(), NS*NC
    std::vector<double> slot_lo, slot_up, stage_lo, stage_up, alat_z, alat_Z;
};
inline TableImages table_images(const SlotTable &t, const ConstraintRows &rows, int B, const double *il, const double *iu, const double *iz,
                                const double *iZ, const double *az, const double *aZ)
{
    const int NS = rows.NS;
    const size_t n = t.entries(), nb = (size_t)NS * NC, np = (size_t)NS * NLAM;
    const bool ib = il && iu, ip = iz && iZ, ia = az && aZ;
    TableImages m;
    m.entries = n; m.stage_rows = nb;
    m.slot_lo.resize((size_t)B * 2 * n); m.slot_up.resize((size_t)B * 2 * n);
    m.stage_lo.resize((size_t)B * (nb + np)); m.stage_up.resize((size_t)B * (nb + np));
    m.alat_z.resize((size_t)B * 2); m.alat_Z.resize((size_t)B * 2);
    for (int b = 0; b < B; b++) {
        double *slo = m.slot_lo.data() + (size_t)b * 2 * n, *sup = m.slot_up.data() + (size_t)b * 2 * n;     // (a table without rows: n = 0)
        for (size_t e = 0; e < n; e++) {
            const int kc = t.kc[e], k = kc >> 4, c = kc & 15;
            double lo = t.lb[e], up = t.ub[e], z = t.zw[e], Z = t.Zw[e];
            if (ib && kc >= 0 && c < 12) {
                if (std::isfinite(lo)) lo = il[((size_t)b * NS + k) * 12 + c];
                if (std::isfinite(up)) up = iu[((size_t)b * NS + k) * 12 + c];
            }
            if (kc >= 0 && Z >= 0.0) {
                const int side = std::isfinite(t.ub[e]) ? 1 : 0;
                if (c == NC) {
                    if (ia) { z = az[b * 2 + side]; Z = aZ[b * 2 + side]; }
                } else if (ip) {
                    const size_t i = ((size_t)b * NS + k) * NLAM + side * NC + c;
                    z = iz[i]; Z = iZ[i];
                }
            }
            slo[e] = lo; sup[e] = up; slo[n + e] = z; sup[n + e] = Z;
        }
        double *tlo = m.stage_lo.data() + (size_t)b * (nb + np), *tup = m.stage_up.data() + (size_t)b * (nb + np);
        for (int k = 0; k < NS; k++)
            for (int c = 0; c < NC; c++) {
                const size_t i = ((size_t)b * NS + k) * 12 + c;
                tlo[k * NC + c] = (ib && c < 12) ? il[i] : rows.lb[k * NC + c];
                tup[k * NC + c] = (ib && c < 12) ? iu[i] : rows.ub[k * NC + c];
            }
        for (size_t i = 0; i < np; i++) {
            tlo[nb + i] = ip ? iz[(size_t)b * np + i] : rows.sz[i];
            tup[nb + i] = ip ? iZ[(size_t)b * np + i] : rows.sZ[i];
        }
        for (int s = 0; s < 2; s++) {
            m.alat_z[b * 2 + s] = ia ? az[b * 2 + s] : rows.alat_sz[s];
            m.alat_Z[b * 2 + s] = ia ? aZ[b * 2 + s] : rows.alat_sZ[s];
        }
    }
    return m;
}

// ---- weights ----

// y = Vx x + Vu u of python/mpc.py:49-58 as one 12x10 selector
inline void cost_selector(double V[NY][NZ])
{
    memset(V, 0, sizeof(double) * NY * NZ);
    for (int i = 0; i < NX; i++) V[i][i] = 1.0;
    V[10][6] = 1.0; V[11][7] = 1.0;
    V[8][8] = 1.0; V[9][9] = 1.0;
    V[10][8] = -1.0; V[11][9] = -1.0;
}

// The QP's weight tables of one stage k < N (cost_scale * V'W_k V, cost_scale * V'W_k) and of the terminal stage (W_e padded with I, W_e).
// ihm2mpc_set_weights and ihm2mpc_set_instance_weights both expand through these: one instance's tables are then those of a batch-shared
// table with its weights bit for bit.
inline void stage_weight_tables(const double *Wk, double cs, double *Hk, double *Gk)
{
    double V[NY][NZ];
    cost_selector(V);
    double VtW[NZ][NY];
    for (int i = 0; i < NZ; i++)
        for (int j = 0; j < NY; j++) {
            double acc = 0;
            for (int l = 0; l < NY; l++) acc += V[l][i] * Wk[l * NY + j];
            VtW[i][j] = acc;
            Gk[i * 12 + j] = cs * acc;
        }
    for (int i = 0; i < NZ; i++)
        for (int j = 0; j < NZ; j++) {
            double acc = 0;
            for (int l = 0; l < NY; l++) acc += VtW[i][l] * V[l][j];
            Hk[i * 10 + j] = cs * acc;
        }
}

inline void terminal_weight_tables(const double *W_e, double *HN, double *GN)
{
    for (int i = 0; i < NX; i++)
        for (int j = 0; j < NX; j++) {
            HN[i * 10 + j] = W_e[i * NX + j];
            GN[i * 12 + j] = W_e[i * NX + j];
        }
    HN[8 * 10 + 8] = 1.0;
    HN[9 * 10 + 9] = 1.0;
}

// true if the 10x10 Hessian of a stage is symmetric (to rounding)
inline bool symmetric10(const double *Hk)
{
    for (int i = 0; i < NZ; i++)
        for (int j = 0; j < i; j++)
            if (fabs(Hk[i * 10 + j] - Hk[j * 10 + i]) > 1e-12 * (1 + fabs(Hk[i * 10 + j]))) return false;
    return true;
}

// true if the blocks of the stages 1..N-1 of a (N, per_stage) table equal stage 0's entry for entry: the QP kernel then keeps one copy
inline bool stages_equal(const double *T, int N, int per_stage)
{
    for (int k = 1; k < N; k++)
        for (int i = 0; i < per_stage; i++)
            if (T[(size_t)k * per_stage + i] != T[i]) return false;
    return true;
}

}  // namespace ihm2
