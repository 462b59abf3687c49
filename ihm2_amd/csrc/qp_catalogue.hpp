// qp_catalogue.hpp -- which instantiations of the QP kernels exist: the lists of the eight objects built from kernels_qp.hip (QP_SET = 0 .. 7),
// entry for entry in their order of preference, the forms every entry of a set is built in, and what both say about the slot tables the
// per-step QP takes.  Plain C++17, no HIP: kernels_qp.hip expands its own set to keys with kernel pointers, the host code (qp_select.hpp,
// api.hip, tools/probes) expands all of them to keys -- from the same macros, so a key cannot say anything else than its kernel's
// template arguments.
//
// WAVE(NSLOT, NSOFT, PATH, UNI) k_qp_wave, BLOCK(NSLOT, UNI, NW) k_qp_block, STEPS(NSLOT, NSOFT, PATH, UNI, IRK, DYN) k_steps.  The
// selection takes the first entry that holds a table, so that an NSLOT comes before the larger ones of the same kind.
#pragma once

#include <utility>
#include <vector>

// A key holds the template parameters as the launch record gives them (include/ihm2mpc.h), kind first; k_qp_block's NSLOT counts the
// slots per thread of its 256-lane table.  nf is not in the record's names: the form of the factor sweep (qp_wave_body: 0 the general
// form, 40 straight-line with the horizon 40 compiled in, -1 straight-line with the run-time horizon) -- same results, so the record
// names the kernel by its other parameters.  full: the form of the slot phases alike (qp_wave_body: FULL; 1 for the tables of
// qp_tables.hpp: slot_table_full), reported beside nf in the record's [15] (qp_select.hpp: encode_launch).
enum { QP_WAVE = 1, QP_BLOCK = 2, QP_STEPS = 3 };
struct QpKey { int kind, nslot, nsoft, path, uni, sqp, irk, dyn, sens, nf, full; };
// The catalogue with its kernels: each object built from kernels_qp.hip returns the table of the instantiations it holds.
struct QpInst { QpKey key; int threads; const void *kernel; };
struct QpTable { const QpInst *inst; int n; };

// QP_SET = 0: the all-hard instantiations (the reference's OCP)
#define QP_INSTANCES_0(WAVE, BLOCK, STEPS)                                                                                                \
    BLOCK(2, 0, 4) BLOCK(2, 1, 4)                                                                                                         \
    WAVE(5, 0, 0, 0) WAVE(5, 0, 0, 1) WAVE(8, 0, 0, 0) WAVE(8, 0, 0, 1) WAVE(10, 0, 0, 0) WAVE(10, 0, 0, 1)                               \
    STEPS(5, 0, 0, 0, 0, 0) STEPS(5, 0, 0, 1, 0, 0) STEPS(5, 0, 0, 1, 1, 0)                                                               \
    STEPS(8, 0, 0, 0, 0, 0) STEPS(8, 0, 0, 1, 0, 0) STEPS(8, 0, 0, 1, 1, 0)                                                               \
    STEPS(10, 0, 0, 1, 0, 0) STEPS(10, 0, 0, 1, 1, 0)
// QP_SET = 1: the soft / track-row instantiations
#define QP_INSTANCES_1(WAVE, BLOCK, STEPS)                                                                                                \
    WAVE(8, 2, 0, 0) WAVE(8, 2, 0, 1) WAVE(10, 4, 0, 0) WAVE(10, 4, 0, 1)                                                                 \
    WAVE(8, 0, 1, 0) WAVE(8, 0, 1, 1) WAVE(8, 3, 1, 0) WAVE(8, 3, 1, 1) WAVE(10, 4, 1, 0) WAVE(10, 4, 1, 1)                               \
    WAVE(8, 0, 2, 1) WAVE(10, 4, 2, 1)                                                                                                    \
    STEPS(8, 2, 0, 1, 0, 0) STEPS(8, 2, 0, 1, 1, 0) STEPS(10, 4, 0, 1, 0, 0) STEPS(10, 4, 0, 1, 1, 0)                                     \
    STEPS(8, 0, 1, 1, 0, 0) STEPS(8, 0, 1, 1, 1, 0) STEPS(8, 3, 1, 1, 0, 0) STEPS(8, 3, 1, 1, 1, 0)                                       \
    STEPS(10, 4, 1, 1, 0, 0) STEPS(10, 4, 1, 1, 1, 0)
// QP_SET = 2: the persistent loop of the dynamic OCP models (all tables)
#define QP_INSTANCES_2(WAVE, BLOCK, STEPS)                                                                                                \
    STEPS(5, 0, 0, 1, 0, 1) STEPS(5, 0, 0, 1, 1, 1) STEPS(8, 0, 0, 1, 0, 1) STEPS(8, 0, 0, 1, 1, 1)                                       \
    STEPS(8, 2, 0, 1, 0, 1) STEPS(8, 2, 0, 1, 1, 1) STEPS(10, 4, 0, 1, 0, 1) STEPS(10, 4, 0, 1, 1, 1)                                     \
    STEPS(8, 0, 1, 1, 0, 1) STEPS(8, 0, 1, 1, 1, 1) STEPS(8, 3, 1, 1, 0, 1) STEPS(8, 3, 1, 1, 1, 1)                                       \
    STEPS(10, 4, 1, 1, 0, 1) STEPS(10, 4, 1, 1, 1, 1)
// QP_SET = 3: the persistent loop with x0 sensitivities (QP_FORMS_3: SENS = 1) for every RTI loop of the sets 0 and 1
#define QP_INSTANCES_3(WAVE, BLOCK, STEPS)                                                                                                \
    STEPS(5, 0, 0, 0, 0, 0) STEPS(5, 0, 0, 1, 0, 0) STEPS(5, 0, 0, 1, 1, 0)                                                               \
    STEPS(8, 0, 0, 0, 0, 0) STEPS(8, 0, 0, 1, 0, 0) STEPS(8, 0, 0, 1, 1, 0)                                                               \
    STEPS(10, 0, 0, 1, 0, 0) STEPS(10, 0, 0, 1, 1, 0)                                                                                     \
    STEPS(8, 2, 0, 1, 0, 0) STEPS(8, 2, 0, 1, 1, 0) STEPS(10, 4, 0, 1, 0, 0) STEPS(10, 4, 0, 1, 1, 0)                                     \
    STEPS(8, 0, 1, 1, 0, 0) STEPS(8, 0, 1, 1, 1, 0) STEPS(8, 3, 1, 1, 0, 0) STEPS(8, 3, 1, 1, 1, 0)                                       \
    STEPS(10, 4, 1, 1, 0, 0) STEPS(10, 4, 1, 1, 1, 0)
// QP_SET = 4: the reference's OCP (all sides hard, batch-shared weights, RTI, RK4, kinematic model) with the factor sweep in its
// straight-line form (qp_wave_body: NF): per-step QP and persistent loop, for the horizon 40 as a compile-time constant and for any
// horizon.  An object of its own (Makefile: without the compiler's own loop unrolling), so that the images of the other sets stay what
// they were.
#define QP_INSTANCES_4(WAVE, BLOCK, STEPS) WAVE(5, 0, 0, 1) STEPS(5, 0, 0, 1, 0, 0)
// QP_SET = 5, IRK = 2: the all-hard kinematic RTI loops with the closed-form actuator lags (IHM2MPC_INTEG_ERK_LAG), in objects of their
// own so that the images of the other sets stay what they were.  SENS = 0 only: ihm2mpc_run_steps_sens launches per step on such a handle.
#define QP_INSTANCES_5(WAVE, BLOCK, STEPS)                                                                                                \
    STEPS(5, 0, 0, 0, 2, 0) STEPS(5, 0, 0, 1, 2, 0) STEPS(8, 0, 0, 0, 2, 0) STEPS(8, 0, 0, 1, 2, 0) STEPS(10, 0, 0, 1, 2, 0)
// QP_SET = 6: ... and the benchmarked table's loop with the straight-line factor sweep, as QP_SET = 4 (Makefile: the same flags)
#define QP_INSTANCES_6(WAVE, BLOCK, STEPS) STEPS(5, 0, 0, 1, 2, 0)
// QP_SET = 7: the list of the set 4 once more -- the same pair, for the horizon 40 only, with the slot phases in their full form
// (qp_wave_body: FULL; qp_tables.hpp: slot_table_full says which tables take it).  No further table fits through it: slot_limits
// does not walk it.  An object of its own with the flags of the set 4, so that the four kernels of that set stay what they were.
#define QP_INSTANCES_7 QP_INSTANCES_4

// ---- the forms of a set: F(SQP, SENS, NF, FULL, entry...) once per form every entry of the set is built in, in this order ----
// A STEPS entry takes every form; a WAVE entry has no SQP mode and takes the forms of the RTI mode; BLOCK exists in the general form,
// where it is listed.
#define QP_FORMS_0(F, ...) F(0, 0, 0, 0, __VA_ARGS__) F(1, 0, 0, 0, __VA_ARGS__)          // both SQP modes
#define QP_FORMS_1 QP_FORMS_0
#define QP_FORMS_2 QP_FORMS_0
#define QP_FORMS_3(F, ...) F(0, 1, 0, 0, __VA_ARGS__)                                   // RTI with SENS = 1
#define QP_FORMS_4(F, ...) F(0, 0, 40, 0, __VA_ARGS__) F(0, 0, -1, 0, __VA_ARGS__)        // RTI, NF = 40 then NF = -1
#define QP_FORMS_5(F, ...) F(0, 0, 0, 0, __VA_ARGS__)                                   // RTI only
#define QP_FORMS_6 QP_FORMS_4
#define QP_FORMS_7(F, ...) F(0, 0, 40, 1, __VA_ARGS__)                                  // RTI, NF = 40, FULL = 1

// the sets, once: X(n) for every QP_SET in catalogue order
#define QP_SETS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)

// QP_ENTRIES(n): the list of the set n, entry-major and form-minor, through three macros the includer defines around it --
//   QP_EMIT_WAVE(NSLOT, NSOFT, PATH, UNI, NF, FULL)    QP_EMIT_BLOCK(NSLOT, UNI, NW)    QP_EMIT_STEPS(NSLOT, NSOFT, PATH, UNI, SQP, IRK, DYN, SENS, NF, FULL)
// -- in the order of the kernels' template parameters.  QP_KEY_* make the key of the same arguments.
#define QP_KEY_WAVE(NS, NO, PT, UN, NF, FU) {QP_WAVE, NS, NO, PT, UN, 0, 0, 0, 0, NF, FU}
#define QP_KEY_BLOCK(NS, UN, NW) {QP_BLOCK, NS, 0, 0, UN, 0, 0, 0, 0, 0, 0}
#define QP_KEY_STEPS(NS, NO, PT, UN, SQ, IR, DY, SE, NF, FU) {QP_STEPS, NS, NO, PT, UN, SQ, IR, DY, SE, NF, FU}
#define QP_WAVE_FORM_0(SE, NF, FU, NS, NO, PT, UN) QP_EMIT_WAVE(NS, NO, PT, UN, NF, FU)
#define QP_WAVE_FORM_1(SE, NF, FU, NS, NO, PT, UN)
#define QP_WAVE_FORM(SQ, SE, NF, FU, NS, NO, PT, UN) QP_WAVE_FORM_##SQ(SE, NF, FU, NS, NO, PT, UN)
#define QP_STEPS_FORM(SQ, SE, NF, FU, NS, NO, PT, UN, IR, DY) QP_EMIT_STEPS(NS, NO, PT, UN, SQ, IR, DY, SE, NF, FU)
#define QP_BLOCK_ENTRY(NS, UN, NW) QP_EMIT_BLOCK(NS, UN, NW)
// (the preprocessor cannot bind a set's forms to an entry kind on the fly: each set names its two pairings)
#define QP_WAVE_0(...) QP_FORMS_0(QP_WAVE_FORM, __VA_ARGS__)
#define QP_WAVE_1(...) QP_FORMS_1(QP_WAVE_FORM, __VA_ARGS__)
#define QP_WAVE_2(...) QP_FORMS_2(QP_WAVE_FORM, __VA_ARGS__)
#define QP_WAVE_3(...) QP_FORMS_3(QP_WAVE_FORM, __VA_ARGS__)
#define QP_WAVE_4(...) QP_FORMS_4(QP_WAVE_FORM, __VA_ARGS__)
#define QP_WAVE_5(...) QP_FORMS_5(QP_WAVE_FORM, __VA_ARGS__)
#define QP_WAVE_6(...) QP_FORMS_6(QP_WAVE_FORM, __VA_ARGS__)
#define QP_WAVE_7(...) QP_FORMS_7(QP_WAVE_FORM, __VA_ARGS__)
#define QP_STEPS_0(...) QP_FORMS_0(QP_STEPS_FORM, __VA_ARGS__)
#define QP_STEPS_1(...) QP_FORMS_1(QP_STEPS_FORM, __VA_ARGS__)
#define QP_STEPS_2(...) QP_FORMS_2(QP_STEPS_FORM, __VA_ARGS__)
#define QP_STEPS_3(...) QP_FORMS_3(QP_STEPS_FORM, __VA_ARGS__)
#define QP_STEPS_4(...) QP_FORMS_4(QP_STEPS_FORM, __VA_ARGS__)
#define QP_STEPS_5(...) QP_FORMS_5(QP_STEPS_FORM, __VA_ARGS__)
#define QP_STEPS_6(...) QP_FORMS_6(QP_STEPS_FORM, __VA_ARGS__)
#define QP_STEPS_7(...) QP_FORMS_7(QP_STEPS_FORM, __VA_ARGS__)
#define QP_ENTRIES_(n) QP_INSTANCES_##n(QP_WAVE_##n, QP_BLOCK_ENTRY, QP_STEPS_##n)
#define QP_ENTRIES(n) QP_ENTRIES_(n)

// the tables of the objects: QpTable ihm2_qp_set0() .. ihm2_qp_set7() (kernels_qp.hip defines the one of its QP_SET)
#define QP_SET_TABLE_(n) ihm2_qp_set##n
#define QP_SET_TABLE(n) QP_SET_TABLE_(n)
#define QP_SET_DECLARE(n) QpTable QP_SET_TABLE(n)();
QP_SETS(QP_SET_DECLARE)
#undef QP_SET_DECLARE

namespace ihm2 {

// Every key of the catalogue with the number of its set, in selection order (set by set, entry-major, form-minor): position i here is
// entry i of the objects' tables laid end to end.  Built once.
struct QpCatKey { QpKey key; int set; };
inline const std::vector<QpCatKey> &catalogue_keys()
{
    static const std::vector<QpCatKey> keys = [] {
        std::vector<QpCatKey> v;
#define QP_EMIT_WAVE(...) QP_KEY_WAVE(__VA_ARGS__),
#define QP_EMIT_BLOCK(...) QP_KEY_BLOCK(__VA_ARGS__),
#define QP_EMIT_STEPS(...) QP_KEY_STEPS(__VA_ARGS__),
#define QP_SET_KEYS(n) { const QpKey set_keys[] = {QP_ENTRIES(n)}; for (const QpKey &k : set_keys) v.push_back({k, n}); }
        QP_SETS(QP_SET_KEYS)
#undef QP_SET_KEYS
#undef QP_EMIT_STEPS
#undef QP_EMIT_BLOCK
#undef QP_EMIT_WAVE
        return v;
    }();
    return keys;
}

// The slot tables the per-step QP takes with the rows of a PATH class (0 none, 1 the track rows, 2 the track rows and the
// lateral-acceleration row): (NSOFT, the largest NSLOT that comes with it) per NSOFT of its k_qp_wave instantiations, in catalogue
// order.  NSOFT = 0: every side hard.  (The further forms of an entry repeat its table: no further table fits through them.)
inline std::vector<std::pair<int, int>> slot_limits(int path)
{
    std::vector<std::pair<int, int>> v;
    for (const QpCatKey &c : catalogue_keys()) {
        const QpKey &w = c.key;
        if (w.kind != QP_WAVE || w.path != path) continue;
        auto p = v.begin();
        while (p != v.end() && p->first != w.nsoft) ++p;
        if (p == v.end()) v.push_back({w.nsoft, w.nslot});
        else if (w.nslot > p->second) p->second = w.nslot;
    }
    return v;
}

// the NSLOT of the instantiations with the slot phases in their full form (qp_tables.hpp: slot_table_full asks for a table of 64 x
// this many slots); 0: the catalogue has none
inline int full_form_nslot()
{
    for (const QpCatKey &c : catalogue_keys())
        if (c.key.kind == QP_WAVE && c.key.full) return c.key.nslot;
    return 0;
}

}  // namespace ihm2
