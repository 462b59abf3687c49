// The problem files of the CPU probes (check_slot_table.cpp, check_qp_select.cpp; tests/test_slot_table.py: problem_text writes them):
// white-space separated tokens
//   name N  lbx ubx (N+1,8)  lbu ubu (N,2)  C (N,2,8)  D (N,2,2)  lg ug (N,2)      -- the arrays of ihm2mpc_set_bounds
//   soft [soft_z soft_Z (N+1,28)]    path lh[2] uh[2]    alat lb ub soft [z[2] Z[2]]      -- soft, path, alat: 0 or 1; [..] only after a 1
//   [uniform_H]      -- 0: stage-varying weights; absent: 1
// and the rows they describe, through the functions api.hip's setters call.
#pragma once

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "qp_tables.hpp"

struct Problem {
    std::string name;
    int N = 0, soft = 0, path = 0, alat = 0, alat_soft = 0, uniform_H = 1;
    std::vector<double> lbx, ubx, lbu, ubu, C, D, lg, ug, soft_z, soft_Z;
    double lh[2] = {0, 0}, uh[2] = {0, 0}, alat_lb = 0, alat_ub = 0, alat_z[2] = {0, 0}, alat_Z[2] = {-1, -1};
};

static bool token(FILE *f, char *buf) { return std::fscanf(f, "%63s", buf) == 1; }
static double number(FILE *f, bool *ok)
{
    char buf[64], *end = buf;
    if (!token(f, buf)) { *ok = false; return 0; }
    const double v = std::strtod(buf, &end);
    if (end == buf || *end) *ok = false;
    return v;
}
static std::vector<double> numbers(FILE *f, size_t n, bool *ok)
{
    std::vector<double> v(n);
    for (double &x : v) x = number(f, ok);
    return v;
}
static bool read_problem(const char *file, Problem *p)
{
    FILE *f = std::fopen(file, "r");
    if (!f) return false;
    char buf[64];
    bool ok = token(f, buf);
    p->name = ok ? buf : "?";
    p->N = (int)number(f, &ok);
    if (!ok || p->N < 2 || p->N > 1024) { std::fclose(f); return false; }
    const size_t N = p->N, NS = N + 1;
    p->lbx = numbers(f, NS * 8, &ok); p->ubx = numbers(f, NS * 8, &ok); p->lbu = numbers(f, N * 2, &ok); p->ubu = numbers(f, N * 2, &ok);
    p->C = numbers(f, N * 16, &ok); p->D = numbers(f, N * 4, &ok);
    p->lg = numbers(f, N * 2, &ok); p->ug = numbers(f, N * 2, &ok);
    p->soft = (int)number(f, &ok);
    if (p->soft) { p->soft_z = numbers(f, NS * NLAM, &ok); p->soft_Z = numbers(f, NS * NLAM, &ok); }
    p->path = (int)number(f, &ok);
    if (p->path) for (double *v : {&p->lh[0], &p->lh[1], &p->uh[0], &p->uh[1]}) *v = number(f, &ok);
    p->alat = (int)number(f, &ok);
    if (p->alat) {
        p->alat_lb = number(f, &ok); p->alat_ub = number(f, &ok);
        p->alat_soft = (int)number(f, &ok);
        if (p->alat_soft) for (double *v : {&p->alat_z[0], &p->alat_z[1], &p->alat_Z[0], &p->alat_Z[1]}) *v = number(f, &ok);
    }
    bool more = true;
    const double uni = number(f, &more);
    if (more) p->uniform_H = (int)uni;
    std::fclose(f);
    return ok;
}

// the rows as api.hip's setters write them: set_bounds, set_path_constraints, set_alat_constraint, set_soft
static ihm2::ConstraintRows rows_of(const Problem &p)
{
    ihm2::ConstraintRows r(p.N + 1);
    r.set_box_rows(p.lbx.data(), p.ubx.data(), p.lbu.data(), p.ubu.data(), p.lg.data(), p.ug.data());
    r.set_track_rows(p.path != 0, p.lh, p.uh);
    if (p.alat) {
        for (int i = 0; i < 2; i++) { r.alat_sz[i] = p.alat_z[i]; r.alat_sZ[i] = p.alat_Z[i]; }
        r.alat_lb = ihm2::bound_or(p.alat_lb, -INFINITY); r.alat_ub = ihm2::bound_or(p.alat_ub, INFINITY);
    }
    r.alat_on = p.alat;
    if (p.soft) { r.sz = p.soft_z; r.sZ = p.soft_Z; }
    return r;
}
