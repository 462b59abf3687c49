// kernels_penalties.hip -- the per-instance slack penalties scattered on the device (ihm2mpc_set_instance_soft_device,
// ihm2mpc_set_instance_alat_soft_device): the twin of the penalty part of ihm2::table_images (qp_tables.hpp), which the host setters run,
// plus the device form of ihm2::find_penalty_mismatch and the fill that stands for "no soft side" in the device adjoint entry.
//
// k_penalty_tables writes the penalty halves of the per-instance images from z, Z in device memory:
//   rows 0..13 (ALAT = false), z, Z (B,NS,28):  zw | Zw of i_slot_lb / i_slot_ub on every slot that is not the a_lat row's, padding included,
//                                               and z | Z of i_st_lb / i_st_ub as given
//   a_lat row  (ALAT = true),  z, Z (B,2):      zw | Zw on the a_lat row's slots, and the (B,2) pairs the cost reads
// A soft slot (kc >= 0 and the SHARED Zw >= 0) takes the instance's value of the side its finite upper bound names -- isfinite(ub) of the
// shared table, as table_images asks -- every other slot the shared zw, Zw.  The pattern is read from the shared slot table the device
// holds (kc, lb | zw, ub | Zw); the bounds halves are not touched.  No arithmetic: every value written is a value read, so the images are
// the host's bit for bit.  z, Z may be the stage image's own penalty halves (stage_out = nullptr: the images are rebuilt from the copy the
// device keeps; strides st_stride), in place.
//
// Mapping: one thread per (instance, entry), entry = slot or (stage, side), consecutive threads consecutive entries: the reads of the
// pattern and every write are coalesced, the gather from z, Z follows the slot order.  Plain vector stores, no LDS, no atomics.
//
// k_penalty_check: one wavefront per instance walks its (stage, side) entries in the order of find_penalty_mismatch and leaves the code
// of the first offence (ihm2mpc_internal.h: ihm2_penalty_code), 0 if none; nothing else is stored.
#include <cmath>

#include "ihm2mpc_internal.h"

namespace {

struct PenaltyTableArgs {
    int B, n, np;                       // instances, slot entries, NS*NLAM
    const int32_t *kc;                  // (n) the shared slot table: stage * 16 + row, -1 = padding
    const double *lo, *up;              // (2,n) lb | zw and ub | Zw of the shared slot table
    const double *z, *Z;                // the instance's values: (B,NS,28) with stride src_stride, or (B,2)
    size_t src_stride;                  // doubles from one instance's z (Z) to the next
    double *slot_lo, *slot_up;          // (B,2,n) the per-instance slot images
    double *stage_lo, *stage_up;        // the penalty halves of the per-instance stage images (stride st_stride) or, ALAT, the (B,2) pairs; nullptr: not written
    size_t st_stride;
};

template <bool ALAT>
__global__ __launch_bounds__(256) void k_penalty_tables(PenaltyTableArgs a)
{
    const size_t E = (size_t)(a.n > a.np ? a.n : a.np);        // entries per instance: the longer of the two tables
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)a.B * E) return;
    const size_t b = idx / E;
    const int e = (int)(idx - b * E);
    const double *z = a.z + b * a.src_stride, *Z = a.Z + b * a.src_stride;
    if (e < a.n) {
        const int kc = a.kc[e], k = kc >> 4, c = kc & 15;
        const bool mine = ALAT ? (kc >= 0 && c == NC) : !(kc >= 0 && c == NC);     // the padding belongs to the rows 0..13
        if (mine) {
            double zw = a.lo[a.n + e], Zw = a.up[a.n + e];
            if (kc >= 0 && Zw >= 0.0) {
                const int side = std::isfinite(a.up[e]) ? 1 : 0;
                const int i = ALAT ? side : k * NLAM + side * NC + c;
                zw = z[i]; Zw = Z[i];
            }
            a.slot_lo[b * 2 * a.n + a.n + e] = zw;
            a.slot_up[b * 2 * a.n + a.n + e] = Zw;
        }
    }
    if (a.stage_lo && e < (ALAT ? 2 : a.np)) {
        a.stage_lo[b * a.st_stride + e] = z[e];
        a.stage_up[b * a.st_stride + e] = Z[e];
    }
}

struct PenaltyCheckArgs {
    int B, np;                          // np: entries per instance, NS*NLAM or 2
    const double *z, *Z;                // (B,np)
    const double *shared_Z;             // (np) the shared table's Z of each side; nullptr: sZ0, sZ1 (the a_lat pair)
    double sZ0, sZ1;
    int32_t *code;                      // (B)
};

// qp_tables.hpp: slot_detail::penalty_side, the four rules in its order; 0 = the side is taken
__device__ inline int penalty_side_kind(double z, double Z, double shared_Z)
{
    if (z != z || Z != Z) return ihm2_penalty_nan;
    if ((Z >= 0.0) != (shared_Z >= 0.0)) return ihm2_penalty_flag;
    if (Z >= 0.0 && !(z >= 0.0)) return ihm2_penalty_negative;
    if (Z >= 0.0 && !(Z + z > 0.0)) return ihm2_penalty_none;
    return 0;
}

__global__ __launch_bounds__(64) void k_penalty_check(PenaltyCheckArgs a)
{
    const int b = blockIdx.x;
    if (b >= a.B) return;
    const int lane = threadIdx.x;
    const double *z = a.z + (size_t)b * a.np, *Z = a.Z + (size_t)b * a.np;
    int code = 0;       // wave-uniform
    for (int e0 = 0; e0 < a.np && !code; e0 += 64) {        // (every lane takes part in the ballot)
        const int e = e0 + lane;
        int kind = 0;
        if (e < a.np) kind = penalty_side_kind(z[e], Z[e], a.shared_Z ? a.shared_Z[e] : (e == 0 ? a.sZ0 : a.sZ1));
        const unsigned long long m = __ballot(kind != 0);
        if (m) {
            const int first = __ffsll((long long)m) - 1;
            code = ihm2_penalty_code(e0 + first, __shfl(kind, first));
        }
    }
    if (lane == 0) a.code[b] = code;
}

// the four penalty gradients of a handle without a soft side: zeros, NaN for instances whose status is neither 0 nor 2 (what the host
// entry fills in after its read-back of the status); per instance n28 doubles in g[0], g[1] and n2 in g[2], g[3], any of them nullptr
struct PenaltyFillArgs { int B; size_t n28, n2; const int32_t *status; double *g[4]; };

__global__ __launch_bounds__(256) void k_penalty_fill(PenaltyFillArgs a)
{
    const size_t per = 2 * (a.n28 + a.n2);
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)a.B * per) return;
    const size_t b = idx / per;
    size_t e = idx - b * per;
    const int st = a.status[b];
    const double v = (st == 0 || st == 2) ? 0.0 : NAN;
    int which = 0;
    size_t n = a.n28;
    if (e >= 2 * a.n28) { e -= 2 * a.n28; which = 2; n = a.n2; }
    if (e >= n) { e -= n; which++; }
    if (a.g[which]) a.g[which][b * n + e] = v;
}

unsigned blocks_of(size_t threads) { return (unsigned)((threads + 255) / 256); }

}  // namespace

void ihm2_launch_penalty_tables(ihm2mpc_handle *h, int alat, const double *z, const double *Z, size_t src_stride, int stage_out)
{
    PenaltyTableArgs a;
    const size_t np = (size_t)h->NS * NLAM, nb = (size_t)h->NS * NC;
    a.B = h->B; a.n = (int)h->slots.entries(); a.np = (int)np;
    a.kc = h->slot_kc; a.lo = h->slot_lb; a.up = h->slot_ub;
    a.z = z; a.Z = Z; a.src_stride = src_stride;
    a.slot_lo = h->i_slot_lb; a.slot_up = h->i_slot_ub;
    if (alat) { a.stage_lo = h->ip.alat_sz; a.stage_up = h->ip.alat_sZ; a.st_stride = 2; }
    else { a.stage_lo = h->i_st_lb + nb; a.stage_up = h->i_st_ub + nb; a.st_stride = nb + np; }
    if (!stage_out) { a.stage_lo = nullptr; a.stage_up = nullptr; }
    const size_t E = std::max((size_t)a.n, np);
    if (alat) hipLaunchKernelGGL(k_penalty_tables<true>, dim3(blocks_of((size_t)h->B * E)), dim3(256), 0, h->stream, a);
    else hipLaunchKernelGGL(k_penalty_tables<false>, dim3(blocks_of((size_t)h->B * E)), dim3(256), 0, h->stream, a);
}

void ihm2_launch_penalty_check(ihm2mpc_handle *h, int alat, const double *z, const double *Z, int32_t *code)
{
    PenaltyCheckArgs a;
    a.B = h->B; a.np = alat ? 2 : h->NS * NLAM;
    a.z = z; a.Z = Z;
    a.shared_Z = alat ? nullptr : h->st_ub + (size_t)h->NS * NC;
    a.sZ0 = h->rows.alat_sZ[0]; a.sZ1 = h->rows.alat_sZ[1];
    a.code = code;
    hipLaunchKernelGGL(k_penalty_check, dim3(h->B), dim3(64), 0, h->stream, a);
}

void ihm2_launch_penalty_fill(ihm2mpc_handle *h, int n_seeds, double *grad_z, double *grad_Z, double *grad_za, double *grad_Za)
{
    PenaltyFillArgs a;
    a.B = h->B; a.n28 = (size_t)n_seeds * h->NS * NLAM; a.n2 = (size_t)n_seeds * h->NS * 2;
    a.status = h->status;
    a.g[0] = grad_z; a.g[1] = grad_Z; a.g[2] = grad_za; a.g[3] = grad_Za;
    hipLaunchKernelGGL(k_penalty_fill, dim3(blocks_of((size_t)h->B * 2 * (a.n28 + a.n2))), dim3(256), 0, h->stream, a);
}
