// The launch decisions (ihm2_amd/csrc/qp_select.hpp, qp_catalogue.hpp) run on the CPU: the QP and step-loop instantiations, the
// linearisation and plant kernels, how ihm2mpc_run_steps proceeds, the launches of the line search's ladder.
//
//   check_qp_select --catalogue
// prints one line per key of the catalogue, in selection order: set kind nslot nsoft path uni sqp irk dyn sens nf full.
//
//   check_qp_select --records
// prints the launch record encode_launch writes for each of those keys alone ("rec R0 .. R15"), then the one note_lin / note_sim write for
// every linearisation and plant kernel, each after its enumerator's name.
//
//   check_qp_select --ladder ALPHA_MIN ALPHA_RED B N
// prints "ladder LENGTH FIRST": ladder_length of the option pair and ladder_first for that length on a handle of B instances and the horizon
// N with the collocation integrator and the backtracking line search; "ladder too_long" for a length above IHM2MPC_LS_MAX_TRIALS.
//
//   check_qp_select "FILE model integrator sim_integrator solver globalization B n_cu sens inst_b block_qp qp_form buffers plant freeze
//                    linearize_cols persistent_rounds" ...
// Each argument is a problem file (problem_file.hpp) followed by the configuration as integers: the IHM2MPC_MODEL_*, IHM2MPC_INTEG_* (twice)
// and nlp_solver_type codes of include/ihm2mpc.h, sqp_globalization, the batch, the device's compute units, sens (1: ihm2mpc_run_steps_sens),
// inst_b (per-instance bounds, with the batch-shared values), block_qp (IHM2MPC_BLOCK_QP), qp_form (IHM2MPC_QP_FORM, 3: unset), the
// buffers that exist as a sum of 1 (collocation tableau), 2 (line-search iterate) and 4 (line-search rollouts), the plant model (-2 .. 2)
// and freeze of ihm2mpc_step / ihm2mpc_run_steps, and the switches IHM2MPC_LINEARIZE_COLS and IHM2MPC_PERSISTENT_ROUNDS.  The slot table is
// laid out as api.hip: rebuild_slots does, a QpSituation filled from it, and every selector runs.  Per argument one line:
//   name  qp POSITION|none LDS_BYTES  steps POSITION|none LDS_BYTES  lin LIN_K_...  sim SIM_K_...  run OUTCOME  rec R0 .. R15
// POSITION: the line of --catalogue, from 0.  OUTCOME (select_run): persistent, no_instantiation, not_resident or refused.  rec: the launch
// record after encode_launch of the QP's key (if any) and of what select_run says of the loop -- the loop's key, or per_step = 1 / 2 as
// ihm2mpc_run_steps writes it, or nothing where the call is refused -- and note_lin / note_sim of the two kernels, as ihm2mpc_step leaves them.
// The last four integers may be left out together: plant model 0, no freeze, both switches off, and the line is the twelve-integer one --
//   name  qp POSITION|none LDS_BYTES  steps POSITION|none LDS_BYTES  rec R0 .. R15
// -- whose record holds the QP's and the loop's keys only.
// By itself the program checks that no two keys of the catalogue are equal in every field.  Exit status 1 on any failure.
// Build: g++ -std=c++17 -fsanitize=address,undefined -I ihm2_amd/csrc tools/probes/check_qp_select.cpp
#include <cstdlib>
#include <cstring>
#include <sstream>

#include "problem_file.hpp"
#include "qp_select.hpp"

using namespace ihm2;

static int fails = 0;

static bool same_key(const QpKey &a, const QpKey &b)
{
    return a.kind == b.kind && a.nslot == b.nslot && a.nsoft == b.nsoft && a.path == b.path && a.uni == b.uni && a.sqp == b.sqp && a.irk == b.irk &&
           a.dyn == b.dyn && a.sens == b.sens && a.nf == b.nf && a.full == b.full;
}

static void check_keys_differ()
{
    const std::vector<QpCatKey> &keys = catalogue_keys();
    for (size_t i = 0; i < keys.size(); i++)
        for (size_t j = i + 1; j < keys.size(); j++)
            if (same_key(keys[i].key, keys[j].key)) { fails++; std::printf("FAIL the keys %zu (set %d) and %zu (set %d) are equal\n", i, keys[i].set, j, keys[j].set); }
}

static void print_catalogue()
{
    for (const QpCatKey &c : catalogue_keys()) {
        const QpKey &k = c.key;
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", c.set, k.kind, k.nslot, k.nsoft, k.path, k.uni, k.sqp, k.irk, k.dyn, k.sens, k.nf, k.full);
    }
}

static void print_record(const int32_t rec[16])
{
    std::printf("rec");
    for (int i = 0; i < 16; i++) std::printf(" %d", (int)rec[i]);
    std::printf("\n");
}

// the record of every key alone, then of every linearisation and plant kernel alone, by the enumerator's name
static void print_records()
{
    for (const QpCatKey &c : catalogue_keys()) {
        int32_t rec[16] = {0};
        encode_launch(rec, c.key);
        print_record(rec);
    }
#define LIN(k) { int32_t rec[16] = {0}; note_lin(rec, k); std::printf("%s ", #k); print_record(rec); }
#define SIM(k) { int32_t rec[16] = {0}; note_sim(rec, k); std::printf("%s ", #k); print_record(rec); }
    LIN(LIN_KERNEL_NONE) LIN(LIN_K_LINEARIZE) LIN(LIN_K_LINEARIZE_DYN) LIN(LIN_K_LINEARIZE_COLS) LIN(LIN_K_LINEARIZE_IRK) LIN(LIN_K_LINEARIZE_LAG)
    SIM(SIM_KERNEL_NONE) SIM(SIM_K_SIM_STEP_KIN) SIM(SIM_K_SIM_STEP) SIM(SIM_K_SIM_IRK) SIM(SIM_K_SIM_STEP_KIN_LAG) SIM(SIM_K_SIM_SENS)
#undef SIM
#undef LIN
}

#define NAME_OF(k) case k: return #k;
static const char *lin_name(LinKernel k)
{
    switch (k) { NAME_OF(LIN_KERNEL_NONE) NAME_OF(LIN_K_LINEARIZE) NAME_OF(LIN_K_LINEARIZE_DYN) NAME_OF(LIN_K_LINEARIZE_COLS) NAME_OF(LIN_K_LINEARIZE_IRK) NAME_OF(LIN_K_LINEARIZE_LAG) }
    return "?";
}
static const char *sim_name(SimKernel k)
{
    switch (k) { NAME_OF(SIM_KERNEL_NONE) NAME_OF(SIM_K_SIM_STEP_KIN) NAME_OF(SIM_K_SIM_STEP) NAME_OF(SIM_K_SIM_IRK) NAME_OF(SIM_K_SIM_STEP_KIN_LAG) NAME_OF(SIM_K_SIM_SENS) }
    return "?";
}
#undef NAME_OF

static void print_choice(const char *what, const QpChoice &c)
{
    if (c.pos < 0) std::printf("  %s none %zu", what, c.lds);
    else std::printf("  %s %d %zu", what, c.pos, c.lds);
}

static bool run(const char *arg)
{
    std::istringstream in(arg);
    std::string file;
    int v[16] = {0};
    in >> file;
    for (int i = 0; i < 12; i++) in >> v[i];
    if (!in) return false;
    // the launch items: all four or none (none: plant 0, no freeze, both switches off, and the line without them)
    const bool launches = static_cast<bool>(in >> v[12]);
    if (launches) for (int i = 13; i < 16; i++) in >> v[i];
    if (launches && !in) return false;
    Problem p;
    if (!read_problem(file.c_str(), &p)) return false;
    // the table as api.hip lays it out (rebuild_slots; per-instance bounds with the shared values leave a full table full)
    const int path = p.alat ? 2 : p.path ? 1 : 0;
    const SlotTable t = lay_out_slots(rows_of(p), slot_limits(path));
    if (!t.fit) return false;
    std::vector<double> CD((size_t)p.N * 20);
    for (int k = 0; k < p.N; k++)
        for (int r = 0; r < 2; r++) {
            for (int j = 0; j < 8; j++) CD[((size_t)k * 2 + r) * 10 + j] = p.C[((size_t)k * 2 + r) * 8 + j];
            for (int j = 0; j < 2; j++) CD[((size_t)k * 2 + r) * 10 + 8 + j] = p.D[((size_t)k * 2 + r) * 2 + j];
        }
    QpSituation s;
    s.N = p.N; s.B = v[5]; s.n_cu = v[6];
    s.model = v[0]; s.integrator_type = v[1]; s.sim_integrator_type = v[2];
    s.nlp_solver_type = v[3]; s.sqp_globalization = v[4];
    s.per_lane = t.per_lane; s.per_blk = t.per_blk; s.nsoft = t.nsoft; s.m_act = t.m_act;
    s.slots_full = slot_table_full(t, full_form_nslot());
    s.path = path;
    s.uni = p.uniform_H && stages_equal(CD.data(), p.N, 20);
    s.inst_b = v[8] != 0; s.block_qp = v[9] != 0;
    s.qp_form = v[10];
    s.irk_tab = (v[11] & 1) != 0; s.ls_x = (v[11] & 2) != 0; s.ls_phi = (v[11] & 4) != 0;
    s.sens_lds = (int)sens_lds_doubles((size_t)p.N);
    s.linearize_cols = v[14] != 0; s.persistent_rounds = v[15] != 0;
    const int sens = v[7], plant = v[12];
    const std::vector<QpCatKey> &keys = catalogue_keys();
    const QpChoice qp = select_qp(s);
    const RunChoice run = select_run(s, sens, v[13] != 0);
    const LinKernel lin = select_linearize(s);
    const SimKernel sim = select_sim(s, plant);
    int32_t rec[16];
    std::memset(rec, 0, sizeof rec);
    if (qp.pos >= 0) encode_launch(rec, keys[qp.pos].key);
    QpKey per_step = {};
    per_step.kind = QP_STEPS;
    if (run.how == RUN_PERSISTENT) encode_launch(rec, keys[run.steps.pos].key);
    else if (run.how != RUN_REFUSED) encode_launch(rec, per_step, run.how);
    static const char *const outcome[] = {"persistent", "no_instantiation", "not_resident", "refused"};
    std::printf("%s", p.name.c_str());
    print_choice("qp", qp);
    print_choice("steps", run.steps);
    std::printf("  ");
    if (launches) {
        note_lin(rec, lin);
        note_sim(rec, sim);
        std::printf("lin %s  sim %s  run %s  ", lin_name(lin), sim_name(sim), outcome[run.how]);
    }
    print_record(rec);
    return true;
}

int main(int argc, char **argv)
{
    check_keys_differ();
    if (argc == 2 && !std::strcmp(argv[1], "--catalogue")) {
        print_catalogue();
        return fails != 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "--records")) {
        print_records();
        return fails != 0;
    }
    if (argc == 6 && !std::strcmp(argv[1], "--ladder")) {
        QpSituation s = {};
        s.integrator_type = IHM2MPC_INTEG_IRK_GL4; s.nlp_solver_type = IHM2MPC_SQP; s.sqp_globalization = IHM2MPC_MERIT_BACKTRACKING;
        s.B = std::atoi(argv[4]); s.N = std::atoi(argv[5]);
        const int n = ladder_length(std::atof(argv[2]), std::atof(argv[3]));
        if (n > IHM2MPC_LS_MAX_TRIALS) std::printf("ladder too_long\n");
        else std::printf("ladder %d %d\n", n, ladder_first(s, n));
        return fails != 0;
    }
    for (int a = 1; a < argc; a++)
        if (!run(argv[a])) { fails++; std::printf("FAIL %s: not a problem file with 12 or 16 integers, or its rows fit no instantiation\n", argv[a]); }
    if (fails) std::printf("%d checks failed\n", fails);
    else std::printf("qp selection: all checks passed\n");
    return fails != 0;
}
