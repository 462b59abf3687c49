// qp_catalogue.hpp -- which instantiations of the QP kernels exist: the lists of the eight objects built from kernels_qp.hip (QP_SET = 0 .. 7),
// entry for entry in their order of preference, and what they say about the slot tables the per-step QP takes.  Plain C++17, no HIP:
// kernels_qp.hip expands its own list to kernel pointers, the host code (api.hip, tools/probes/check_slot_table.cpp) expands them to
// numbers.
//
// WAVE(NSLOT, NSOFT, PATH, UNI) k_qp_wave, BLOCK(NSLOT, UNI, NW) k_qp_block, STEPS(NSLOT, NSOFT, PATH, UNI, IRK, DYN) k_steps in both SQP
// modes (QP_SET = 3: in the RTI mode, with SENS = 1).  The selection takes the first entry that holds a table, so that an NSLOT comes
// before the larger ones of the same kind.
#pragma once

#include <utility>
#include <vector>

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
// QP_SET = 3: the persistent loop with x0 sensitivities (SENS = 1) for every RTI loop of the sets 0 and 1
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

namespace ihm2 {

// The slot tables the per-step QP takes with the rows of a PATH class (0 none, 1 the track rows, 2 the track rows and the
// lateral-acceleration row): (NSOFT, the largest NSLOT that comes with it) per NSOFT of its k_qp_wave instantiations, in catalogue
// order.  NSOFT = 0: every side hard.
inline std::vector<std::pair<int, int>> slot_limits(int path)
{
    struct Wave { int nslot, nsoft, path; };
#define IHM2_CATALOGUE_WAVE(NS, NO, PT, UN) {NS, NO, PT},
#define IHM2_CATALOGUE_SKIP(...)
#define IHM2_CATALOGUE_SET(n) QP_INSTANCES_##n(IHM2_CATALOGUE_WAVE, IHM2_CATALOGUE_SKIP, IHM2_CATALOGUE_SKIP)
    static const Wave waves[] = {IHM2_CATALOGUE_SET(0) IHM2_CATALOGUE_SET(1) IHM2_CATALOGUE_SET(2) IHM2_CATALOGUE_SET(3)
                                 IHM2_CATALOGUE_SET(4) IHM2_CATALOGUE_SET(5) IHM2_CATALOGUE_SET(6)};
#undef IHM2_CATALOGUE_SET
#undef IHM2_CATALOGUE_SKIP
#undef IHM2_CATALOGUE_WAVE
    std::vector<std::pair<int, int>> v;
    for (const Wave &w : waves) {
        if (w.path != path) continue;
        auto p = v.begin();
        while (p != v.end() && p->first != w.nsoft) ++p;
        if (p == v.end()) v.push_back({w.nsoft, w.nslot});
        else if (w.nslot > p->second) p->second = w.nslot;
    }
    return v;
}

}  // namespace ihm2
