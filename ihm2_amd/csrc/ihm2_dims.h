// ihm2_dims.h -- the dimensions of the OCP and of the QP's constraint-slot table.  No HIP: ihm2mpc_internal.h takes them for the kernels
// and the handle, qp_tables.hpp for the host code that a plain C++ compiler builds as well.
#pragma once

#define NX 8
#define NU 2
#define NZ 10
#define NY 12
#define NG 2
#define NH 2
#define NC 14   // two-sided constraint rows per stage: 8 state boxes, 2 input boxes, 2 general rows, 2 track rows
#define NLAM 28
#define MAX_SLOTS 640   // 10 per lane
