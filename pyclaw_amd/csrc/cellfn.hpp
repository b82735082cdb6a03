// cellfn.hpp -- user-written cell functions: a C++ function body given as text, compiled at run time for the library's
// architecture and launched as one pointwise pass over the interior cells of the resident arrays (step_src, dq_src and
// start_step of the Python drivers).
//
// The wrapper kernel below is kept as text.  The user's preamble and body are spliced into it, MEQN / MAUX / NDIM and
// the kind arrive as -D constants (q[MEQN] and aux[MAUX] unroll into registers), and hiprtc compiles the whole for
// PCL_ARCH without asking any device.  One lane = one interior cell, x fastest, 256 threads per workgroup; ghost cells
// are never written.  A component is stored only where its bits differ from the bits that were loaded: for a
// component the body never assigns the comparison folds at compile time, and the store and then the load disappear
// from the code object (the built-in source kernels leave such planes alone in the same way).
//
// Neighbour reads (-DREACH=n, n > 0; pcl_cellfn_compile_reach): the body also gets qn(m, di, dj, dk) and auxn(...),
// component m of the cell at that index offset.  Every read of q, the lane's own cell included, then comes from
// pcl_cell_args.snap -- a copy of the selected register that pcl_cellfn_apply takes in front of the launch (dq_src: the
// register itself, which that kind cannot write) -- and the stores go to the register: every lane sees the state as it
// was when the launch began.  Offsets are clamped to [-REACH, REACH] and REACH <= mbc is checked at the launch, so a read
// lands in the ghosted block whatever the body passes; the ghost cells it may land in are the caller's to fill.  Without
// -DREACH the text compiles to what it compiled to before there was one (qn / auxn are stubs that fail to instantiate
// with a message that names reach).
//
// A fourth kind, the boundary condition (PCL_CELLFN_BC; pyclaw.CellBC), has a wrapper of its own further
// down: one lane = one ghost cell of one side, the body's only neighbour reads go inward along the lane's own normal line.
//
// A fifth wrapper, the functional (pcl_cellfn_compile_reduce; pyclaw.CellFunctional), stores nothing into
// the state: every lane evaluates the body into f[NOUT] and the workgroup reduces those to NOUT partials (kCellfnReduce*
// below).  Its kind value is internal: pcl_cellfn_compile knows the kinds 1..4 alone.
//
// libhiprtc is dlopen()ed on first use, like librccl in halo.hpp: a library without it loads and runs every other path.
#pragma once
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#ifndef PCL_ARCH
#define PCL_ARCH "gfx950"
#endif

#define PCL_CELLFN_MAX_PARAMS 16
#define PCL_CELLFN_MAX_NOUT 8
// the kind a handle of pcl_cellfn_compile_reduce carries; not a kind of pcl_cellfn_compile (the public ones are 1..4)
#define PCL_CELLFN_KIND_REDUCE 5

// by-value argument of the wrapper kernel; the text below declares the same struct for the device compile
struct pcl_cell_args {
    double *q;          // the selected register
    double *dq;         // dq_src: the increment register; functional: the workgroups' partials, [NOUT][workgroups]
    double *aux;
    long pitch, plane, slab;        // doubles between rows, components and (3-D) k-planes
    int n[3];           // interior cells of this block
    int mbc;
    int nstart[3];      // global index of this block's first interior cell
    int pad_;
    double lower[3], d[3];
    double t, dt;
    double p[PCL_CELLFN_MAX_PARAMS];
    // reach > 0 only (a reach = 0 launch passes the bytes in front of it): what qn() reads, laid out like q -- the
    // snapshot of the selected register taken in front of the launch, or (dq_src, q const) the register itself
    const double *snap;
};

// the same for the boundary-condition wrapper (pcl_cellbc below)
struct pcl_cellbc_args {
    double *q;          // the selected register
    const double *aux;
    long pitch, plane, slab;
    int n[3];           // interior cells of this block
    int mbc;
    int nstart[3];
    int idim, side;     // the side this launch fills
    int ext[3];         // cells with ghosts: the transverse extent of the launch
    double lower[3], d[3];
    double t;
    double p[PCL_CELLFN_MAX_PARAMS];
};

namespace pcl {

static const char *const kCellfnHead = R"PCLSRC(
#ifndef REACH
#define REACH 0
#endif
struct pcl_cell {
    double t, dt;
    int i[NDIM];
    double x[NDIM];
    double d[NDIM];
};
struct pcl_cell_args {
    double *q;
    double *dq;
    double *aux;
    long pitch, plane, slab;
    int n[3];
    int mbc;
    int nstart[3];
    int pad_;
    double lower[3], d[3];
    double t, dt;
    double p[16];
#if REACH > 0
    const double *snap;
#endif
};
#define PCL_MAUXN (MAUX > 0 ? MAUX : 1)
#if KIND == 2 || KIND == 5
#define PCL_Q_QUAL const
#else
#define PCL_Q_QUAL
#endif
#if WRITES_AUX
#define PCL_AUX_QUAL
#else
#define PCL_AUX_QUAL const
#endif
#if REACH > 0
// neighbour reads: q and aux point at the lane's own cell of the array being read.  Every offset is clamped to
// [-REACH, REACH] and m to the components there are, so with REACH <= mbc (pcl_cellfn_apply) no argument reaches
// outside the ghosted block; for literal arguments the clamps fold away.
struct pcl_near {
    const double *q, *aux;
    long pitch, plane, slab;
    static __device__ __forceinline__ int cl(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
    __device__ __forceinline__ long at(int di, int dj, int dk) const {
        long o = cl(di, -REACH, REACH);
        if (NDIM > 1) o += (long)cl(dj, -REACH, REACH) * pitch;
        if (NDIM > 2) o += (long)cl(dk, -REACH, REACH) * slab;
        return o;
    }
    __device__ __forceinline__ double qn(int m, int di, int dj, int dk) const {
        return q[cl(m, 0, MEQN - 1) * plane + at(di, dj, dk)];
    }
    __device__ __forceinline__ double auxn(int m, int di, int dj, int dk) const {
        return MAUX > 0 ? aux[cl(m, 0, PCL_MAUXN - 1) * plane + at(di, dj, dk)] : 0.0;
    }
};
#define PCL_NEAR_PARAM , const pcl_near &pcl_nb
#else
// reach = 0: the names exist so that a body which uses them is told why it does not compile
template <class...> struct pcl_no_reach { static constexpr bool value = false; };
template <class... A> __device__ double qn(A...) {
    static_assert(pcl_no_reach<A...>::value, "qn() reads neighbour cells: give the cell function reach > 0");
    return 0.0;
}
template <class... A> __device__ double auxn(A...) {
    static_assert(pcl_no_reach<A...>::value, "auxn() reads neighbour cells: give the cell function reach > 0");
    return 0.0;
}
#define PCL_NEAR_PARAM
#endif
)PCLSRC";

// between preamble and body
static const char *const kCellfnOpen = R"PCLSRC(
__device__ __forceinline__ void pcl_cell_body(PCL_Q_QUAL double (&q)[MEQN], double (&dq)[MEQN],
                                              PCL_AUX_QUAL double (&aux)[PCL_MAUXN], const pcl_cell &c,
                                              const double (&p)[16] PCL_NEAR_PARAM) {
#if REACH > 0
    const auto qn = [&pcl_nb](int m, int di, int dj = 0, int dk = 0) { return pcl_nb.qn(m, di, dj, dk); };
    (void)qn;
#if MAUX > 0
    const auto auxn = [&pcl_nb](int m, int di, int dj = 0, int dk = 0) { return pcl_nb.auxn(m, di, dj, dk); };
    (void)auxn;
#endif
#endif
)PCLSRC";

static const char *const kCellfnTail = R"PCLSRC(
}
#line 1 "pcl_cellfn_wrapper"
__device__ __forceinline__ bool pcl_bits_differ(double a, double b) {
    return __builtin_bit_cast(unsigned long long, a) != __builtin_bit_cast(unsigned long long, b);
}
extern "C" __global__ void __launch_bounds__(256) pcl_cellfn(const pcl_cell_args a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n[0]) return;
    const int j = NDIM > 1 ? (int)blockIdx.y : 0, k = NDIM > 2 ? (int)blockIdx.z : 0;
    long g = i + a.mbc;
    if (NDIM > 1) g += (long)(j + a.mbc) * a.pitch;
    if (NDIM > 2) g += (long)(k + a.mbc) * a.slab;
    pcl_cell c;
    c.t = a.t;
    c.dt = a.dt;
    const int loc[3] = {i, j, k};
    for (int n = 0; n < NDIM; n++) {
        c.i[n] = loc[n] + a.nstart[n];
        c.d[n] = a.d[n];
        c.x[n] = a.lower[n] + (c.i[n] + 0.5) * a.d[n];
    }
    double q0[MEQN], q[MEQN], dq[MEQN], aux0[PCL_MAUXN], aux[PCL_MAUXN];
#if REACH > 0
    // Every read of q, the lane's own cell included, comes from a.snap: the state as it was when the launch began.  The
    // stores below go to a.q (a.dq), another array, so no lane sees what a lane of this launch stored.
    for (int m = 0; m < MEQN; m++) { q0[m] = a.snap[m * a.plane + g]; q[m] = q0[m]; dq[m] = 0.0; }
    for (int m = 0; m < PCL_MAUXN; m++) { aux0[m] = MAUX > 0 ? a.aux[m * a.plane + g] : 0.0; aux[m] = aux0[m]; }
    pcl_near nb;
    nb.q = a.snap + g;
    nb.aux = MAUX > 0 ? a.aux + g : nullptr;
    nb.pitch = a.pitch; nb.plane = a.plane; nb.slab = a.slab;
    pcl_cell_body(q, dq, aux, c, a.p, nb);
#else
    for (int m = 0; m < MEQN; m++) { q0[m] = a.q[m * a.plane + g]; q[m] = q0[m]; dq[m] = 0.0; }
    for (int m = 0; m < PCL_MAUXN; m++) { aux0[m] = MAUX > 0 ? a.aux[m * a.plane + g] : 0.0; aux[m] = aux0[m]; }
    pcl_cell_body(q, dq, aux, c, a.p);
#endif
#if KIND == 2
    for (int m = 0; m < MEQN; m++) {
        const double old = a.dq[m * a.plane + g];
        const double now = old + dq[m];
        if (pcl_bits_differ(now, old)) a.dq[m * a.plane + g] = now;
    }
#else
    for (int m = 0; m < MEQN; m++)
        if (pcl_bits_differ(q[m], q0[m])) a.q[m * a.plane + g] = q[m];
#endif
#if WRITES_AUX
    for (int m = 0; m < MAUX; m++)
        if (pcl_bits_differ(aux[m], aux0[m])) a.aux[m * a.plane + g] = aux[m];
#endif
}
)PCLSRC";

// ---- the boundary-condition kind ------------------------------------------------------------------------------------
// One lane = one ghost cell of side (idim, side): mbc layers times the whole ghosted extent of the transverse
// dimensions, corner cells included (the reference hands its callback the full qbc, and the y fill sees the x-filled
// ghosts).  The lanes are numbered x fastest over that box, 256 to a workgroup: a y or z side stores whole rows
// coalesced; an x side is mbc columns wide, so a wavefront touches 64 / mbc rows -- strided, and O(perimeter).
// idim and side are run-time fields: one code object serves every side of a solver.
// qin(m, r) / auxin(m, r) read component m of the cell r cells inward from the boundary face on the lane's own normal
// line, r clamped to the interior [0, n[idim] - 1]: the address is always an interior cell of the block, which no lane
// of a side launch writes.
static const char *const kCellbcHead = R"PCLSRC(
struct pcl_cell {
    double t;
    int idim, side, g;
    int i[NDIM];
    double x[NDIM];
    double d[NDIM];
};
struct pcl_cellbc_args {
    double *q;
    const double *aux;
    long pitch, plane, slab;
    int n[3];
    int mbc;
    int nstart[3];
    int idim, side;
    int ext[3];
    double lower[3], d[3];
    double t;
    double p[16];
};
#define PCL_MAUXN (MAUX > 0 ? MAUX : 1)
struct pcl_inward {
    const double *q, *aux;
    long plane, line, stride;       // line: the lane's cell offset with the normal coordinate at the first ghosted cell
    int n, mbc, side;
    __device__ __forceinline__ long at(int r) const {
        r = r < 0 ? 0 : r > n - 1 ? n - 1 : r;
        return line + (long)(side == 0 ? mbc + r : mbc + n - 1 - r) * stride;
    }
    __device__ __forceinline__ double qin(int m, int r) const { return q[m * plane + at(r)]; }
    __device__ __forceinline__ double auxin(int m, int r) const { return MAUX > 0 ? aux[m * plane + at(r)] : 0.0; }
};
)PCLSRC";

static const char *const kCellbcOpen = R"PCLSRC(
__device__ __forceinline__ void pcl_cell_body(double (&q)[MEQN], const double (&aux)[PCL_MAUXN], const pcl_cell &c,
                                              const double (&p)[16], const pcl_inward &pcl_in) {
    const auto qin = [&pcl_in](int m, int r) { return pcl_in.qin(m, r); };
    const auto auxin = [&pcl_in](int m, int r) { return pcl_in.auxin(m, r); };
    (void)qin; (void)auxin;
)PCLSRC";

static const char *const kCellbcTail = R"PCLSRC(
}
#line 1 "pcl_cellbc_wrapper"
__device__ __forceinline__ bool pcl_bits_differ(double a, double b) {
    return __builtin_bit_cast(unsigned long long, a) != __builtin_bit_cast(unsigned long long, b);
}
extern "C" __global__ void __launch_bounds__(256) pcl_cellbc(const pcl_cellbc_args a) {
    // the box of this side in ghosted indices: mbc cells along idim, everything across
    int e[3] = {1, 1, 1};
    for (int n = 0; n < NDIM; n++) e[n] = n == a.idim ? a.mbc : a.ext[n];
    const long lane = (long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= (long)e[0] * e[1] * e[2]) return;
    int pos[3];
    pos[0] = (int)(lane % e[0]);
    pos[1] = (int)(lane / e[0] % e[1]);
    pos[2] = (int)(lane / ((long)e[0] * e[1]));
    const long st[3] = {1, a.pitch, a.slab};
    pcl_cell c;
    c.t = a.t;
    c.idim = a.idim;
    c.side = a.side;
    c.g = 0;
    pcl_inward in;
    in.q = a.q; in.aux = a.aux; in.plane = a.plane; in.line = 0; in.stride = 1;
    in.n = 1; in.mbc = a.mbc; in.side = a.side;
    long g = 0;
    for (int n = 0; n < NDIM; n++) {
        int k = pos[n];             // ghosted index of the cell along n
        if (n == a.idim) {
            c.g = a.side == 0 ? a.mbc - 1 - k : k;
            if (a.side) k += a.mbc + a.n[n];
            in.stride = st[n];
            in.n = a.n[n];
        } else {
            in.line += k * st[n];
        }
        g += k * st[n];
        c.i[n] = k - a.mbc + a.nstart[n];
        c.d[n] = a.d[n];
        c.x[n] = a.lower[n] + (c.i[n] + 0.5) * a.d[n];
    }
    double q0[MEQN], q[MEQN], aux[PCL_MAUXN];
    for (int m = 0; m < MEQN; m++) { q0[m] = a.q[m * a.plane + g]; q[m] = q0[m]; }
    for (int m = 0; m < PCL_MAUXN; m++) aux[m] = MAUX > 0 ? a.aux[m * a.plane + g] : 0.0;
    pcl_cell_body(q, aux, c, a.p, in);
    for (int m = 0; m < MEQN; m++)
        if (pcl_bits_differ(q[m], q0[m])) a.q[m * a.plane + g] = q[m];
}
)PCLSRC";

// ---- the functional: per-cell integrands reduced over the interior ------------------------------------------------------
// The head is the cell functions' (q and aux const, qn / auxn read the register itself).  One lane = one interior cell as
// above, but no lane leaves early: a lane beyond the row contributes the identity of each output's operation (+0, -inf,
// +inf).  The order of the combination is fixed by the block's shape alone -- the same bits on every call:
//   1. across the wavefront, a butterfly of 6 cross-lane exchanges at distances 1, 2, 4, ... 32 (a + b and b + a have the
//      same bits, so every lane of a pair holds the same value after each exchange);
//   2. across the workgroup's four wavefronts through LDS, by thread 0 in wavefront order 0, 1, 2, 3;
//   3. thread 0 stores the NOUT partials of workgroup w at a.dq[m * workgroups + w] with plain vector stores; the library's
//      reduce_partials_kernel (kernels.hip) combines those, again in a fixed order.
// No atomics and no counters: nothing depends on which workgroup finishes first.  PCL_OPS is the comma-separated list of
// the NOUT operations (PCL_REDUCE_*): 0 sum, 1 sum of |f|, 2 max, 3 min; max / min are fmax / fmin, which pass over a NaN.
static const char *const kCellfnReduceOpen = R"PCLSRC(
__device__ __forceinline__ void pcl_cell_body(const double (&q)[MEQN], double (&f)[NOUT],
                                              const double (&aux)[PCL_MAUXN], const pcl_cell &c,
                                              const double (&p)[16] PCL_NEAR_PARAM) {
#if REACH > 0
    const auto qn = [&pcl_nb](int m, int di, int dj = 0, int dk = 0) { return pcl_nb.qn(m, di, dj, dk); };
    (void)qn;
#if MAUX > 0
    const auto auxn = [&pcl_nb](int m, int di, int dj = 0, int dk = 0) { return pcl_nb.auxn(m, di, dj, dk); };
    (void)auxn;
#endif
#endif
)PCLSRC";

static const char *const kCellfnReduceTail = R"PCLSRC(
}
#line 1 "pcl_cellfn_wrapper"
__device__ __forceinline__ double pcl_red_identity(int op) {
    return op == 2 ? -__builtin_huge_val() : op == 3 ? __builtin_huge_val() : 0.0;
}
__device__ __forceinline__ double pcl_red_combine(int op, double a, double b) {
    return op == 2 ? fmax(a, b) : op == 3 ? fmin(a, b) : a + b;
}
extern "C" __global__ void __launch_bounds__(256) pcl_cellfn_red(const pcl_cell_args a) {
    constexpr int ops[NOUT] = {PCL_OPS};
    __shared__ double part[4][NOUT];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int j = NDIM > 1 ? (int)blockIdx.y : 0, k = NDIM > 2 ? (int)blockIdx.z : 0;
    double f[NOUT];
    for (int m = 0; m < NOUT; m++) f[m] = pcl_red_identity(ops[m]);
    if (i < a.n[0]) {
        long g = i + a.mbc;
        if (NDIM > 1) g += (long)(j + a.mbc) * a.pitch;
        if (NDIM > 2) g += (long)(k + a.mbc) * a.slab;
        pcl_cell c;
        c.t = a.t;
        c.dt = a.dt;
        const int loc[3] = {i, j, k};
        for (int n = 0; n < NDIM; n++) {
            c.i[n] = loc[n] + a.nstart[n];
            c.d[n] = a.d[n];
            c.x[n] = a.lower[n] + (c.i[n] + 0.5) * a.d[n];
        }
        double q[MEQN], aux[PCL_MAUXN], v[NOUT];
        for (int m = 0; m < MEQN; m++) q[m] = a.q[m * a.plane + g];
        for (int m = 0; m < PCL_MAUXN; m++) aux[m] = MAUX > 0 ? a.aux[m * a.plane + g] : 0.0;
        for (int m = 0; m < NOUT; m++) v[m] = 0.0;
#if REACH > 0
        pcl_near nb;
        nb.q = a.snap + g;          // the register itself: q is const, the launch stores nothing into it
        nb.aux = MAUX > 0 ? a.aux + g : nullptr;
        nb.pitch = a.pitch; nb.plane = a.plane; nb.slab = a.slab;
        pcl_cell_body(q, v, aux, c, a.p, nb);
#else
        pcl_cell_body(q, v, aux, c, a.p);
#endif
        for (int m = 0; m < NOUT; m++) f[m] = ops[m] == 1 ? fabs(v[m]) : v[m];
    }
    for (int m = 0; m < NOUT; m++) {
        double v = f[m];
        for (int w = 1; w < 64; w <<= 1) v = pcl_red_combine(ops[m], v, __shfl_xor(v, w, 64));
        f[m] = v;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int m = 0; m < NOUT; m++) part[wave][m] = f[m];
    __syncthreads();
    if (threadIdx.x == 0) {
        const long nwg = (long)gridDim.x * gridDim.y * gridDim.z;
        const long wg = blockIdx.x + (long)gridDim.x * (blockIdx.y + (long)gridDim.y * blockIdx.z);
        for (int m = 0; m < NOUT; m++) {
            double v = part[0][m];
            for (int w = 1; w < 4; w++) v = pcl_red_combine(ops[m], v, part[w][m]);
            a.dq[m * nwg + wg] = v;
        }
    }
}
)PCLSRC";

static inline const char *cellfn_kind_name(int kind) {
    return kind == 1 ? "step_src" : kind == 2 ? "dq_src" : kind == 3 ? "start_step" : kind == 4 ? "bc" : nullptr;
}
// the same for messages about any live handle: a functional's kind is none of pcl_cellfn_compile's
static inline const char *cellfn_kind_label(int kind) {
    return kind == PCL_CELLFN_KIND_REDUCE ? "functional" : cellfn_kind_name(kind) ? cellfn_kind_name(kind) : "unknown";
}
// the __global__ function of a kind's wrapper
static inline const char *cellfn_entry_name(int kind) {
    return kind == 4 ? "pcl_cellbc" : kind == PCL_CELLFN_KIND_REDUCE ? "pcl_cellfn_red" : "pcl_cellfn";
}

// ---- libhiprtc, loaded on first use ---------------------------------------------------------------------------
struct HiprtcApi {
    bool ok = false;
    decltype(&hiprtcCreateProgram) hiprtcCreateProgram = nullptr;
    decltype(&hiprtcCompileProgram) hiprtcCompileProgram = nullptr;
    decltype(&hiprtcGetProgramLogSize) hiprtcGetProgramLogSize = nullptr;
    decltype(&hiprtcGetProgramLog) hiprtcGetProgramLog = nullptr;
    decltype(&hiprtcGetCodeSize) hiprtcGetCodeSize = nullptr;
    decltype(&hiprtcGetCode) hiprtcGetCode = nullptr;
    decltype(&hiprtcDestroyProgram) hiprtcDestroyProgram = nullptr;
    decltype(&hiprtcGetErrorString) hiprtcGetErrorString = nullptr;
    decltype(&hiprtcAddNameExpression) hiprtcAddNameExpression = nullptr;      // cellrp.hpp: the symbols of template kernels
    decltype(&hiprtcGetLoweredName) hiprtcGetLoweredName = nullptr;
};
static inline HiprtcApi &hiprtc_api() {
    static HiprtcApi a;
    return a;
}

// PCL_HIPRTC_LIB names the one file to open instead (a private ROCm tree; tests point it at a file that does not
// exist).  Otherwise: the versioned sonames, the plain name, then the lib directory the HIP runtime itself was loaded from.
static inline int hiprtc_load(std::string &err) {
    HiprtcApi &a = hiprtc_api();
    if (a.ok) return 0;
    void *h = nullptr;
    std::string tried;
    auto open = [&](const std::string &name) {
        if (h) return;
        h = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!h) tried += (tried.empty() ? "" : "; ") + std::string(dlerror());
    };
    if (const char *over = getenv("PCL_HIPRTC_LIB")) {
        open(over);
    } else {
        open("libhiprtc.so.7");
        open("libhiprtc.so.6");
        open("libhiprtc.so");
        Dl_info info;
        if (!h && dladdr((void *)&hipGetDeviceCount, &info) && info.dli_fname) {
            std::string dir(info.dli_fname);
            const size_t slash = dir.rfind('/');
            if (slash != std::string::npos) open(dir.substr(0, slash + 1) + "libhiprtc.so");
        }
    }
    if (!h) { err = "cell functions need libhiprtc, which could not be opened: " + tried; return -1; }
#define PCL_SYM(name)                                                      \
    a.name = (decltype(a.name))dlsym(h, #name);                            \
    if (!a.name) { err = "libhiprtc lacks " #name; return -1; }
    PCL_SYM(hiprtcCreateProgram) PCL_SYM(hiprtcCompileProgram) PCL_SYM(hiprtcGetProgramLogSize)
    PCL_SYM(hiprtcGetProgramLog) PCL_SYM(hiprtcGetCodeSize) PCL_SYM(hiprtcGetCode) PCL_SYM(hiprtcDestroyProgram)
    PCL_SYM(hiprtcGetErrorString) PCL_SYM(hiprtcAddNameExpression) PCL_SYM(hiprtcGetLoweredName)
#undef PCL_SYM
    a.ok = true;
    return 0;
}

}  // namespace pcl

// ---- compiled functions, cached per process --------------------------------------------------------------------
struct pcl_cellfn {
    long id = 0;                // never reused: the solvers' loaded modules are keyed by it
    int kind = 0, meqn = 0, maux = 0, ndim = 0, math = 0, writes_aux = 0, reach = 0;
    int nout = 0, ops[PCL_CELLFN_MAX_NOUT] = {0, 0, 0, 0, 0, 0, 0, 0};      // a functional's outputs (PCL_REDUCE_*)
    int refs = 0;
    std::string key;
    std::vector<char> code;     // the code object
};

struct pcl_cellrp;      // a compiled Riemann solver (cellrp.hpp): same cache, same counters

namespace pcl {

// No destructor work that touches HIP: the cache holds host memory only (the modules loaded from it belong to the
// solver handles and are unloaded by pcl_destroy).
struct CellfnCache {
    std::mutex mu;
    std::map<std::string, pcl_cellfn *> by_key;
    std::map<const pcl_cellfn *, long> live;
    std::map<std::string, pcl_cellrp *> rp_by_key;
    std::map<const pcl_cellrp *, long> rp_live;
    long next_id = 1, compiles = 0, hits = 0;
};
static inline CellfnCache &cellfn_cache() {
    static CellfnCache *c = new CellfnCache();     // never destroyed: handles may outlive static destruction order
    return *c;
}

static inline std::string cellfn_key(int kind, const char *body, const char *preamble, int meqn, int maux, int ndim, int math,
                                     int writes_aux, int reach) {
    // (reach = 0 keeps the key it always had: that one starts with a digit)
    std::string k = reach > 0 ? "reach=" + std::to_string(reach) + ";" : std::string();
    k += std::to_string(kind) + "," + std::to_string(meqn) + "," + std::to_string(maux) + "," +
         std::to_string(ndim) + "," + std::to_string(math) + "," + std::to_string(writes_aux) + ",";
    k += std::to_string(strlen(preamble)) + ":";
    k += preamble;
    k += body;
    return k;
}

// One hiprtc compile, for the cell functions here and the Riemann solvers of cellrp.hpp: what goes in ...
struct HiprtcJob {
    std::string src;
    const char *name = "";                  // the program's name
    int nheaders = 0;                       // named headers the text includes (none: a cell function)
    const char **header_texts = nullptr, **header_names = nullptr;
    std::vector<std::string> exprs;         // name expressions: template kernels whose lowered names are wanted
    std::vector<std::string> opts;          // the compiler's options, in order
    std::string what;                       // "<what> does not compile: ..." in front of the log
    std::string dump;                       // PCL_CELLFN_DUMP keeps the code object as <dir>/<dump>_<*dump_seq>.co
    int *dump_seq = nullptr;
};
// ... and what comes out: the code object and the lowered name of every expression.  0 = ok, else err holds the log
static inline int hiprtc_compile(const HiprtcJob &job, std::vector<char> &code, std::vector<std::string> &lowered, std::string &err) {
    if (hiprtc_load(err)) return -1;
    HiprtcApi &a = hiprtc_api();
    hiprtcProgram prog = nullptr;
    hiprtcResult r = a.hiprtcCreateProgram(&prog, job.src.c_str(), job.name, job.nheaders, job.header_texts, job.header_names);
    if (r != HIPRTC_SUCCESS) { err = std::string("hiprtcCreateProgram: ") + a.hiprtcGetErrorString(r); return -1; }
    const auto fails = [&](const std::string &msg) {
        err = msg;
        a.hiprtcDestroyProgram(&prog);
        return -1;
    };
    for (const std::string &e : job.exprs) {
        r = a.hiprtcAddNameExpression(prog, e.c_str());
        if (r != HIPRTC_SUCCESS) return fails(std::string("hiprtcAddNameExpression: ") + a.hiprtcGetErrorString(r));
    }
    std::vector<const char *> opts;
    for (const std::string &o : job.opts) opts.push_back(o.c_str());
    r = a.hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
    if (r != HIPRTC_SUCCESS) {
        size_t n = 0;
        std::string log;
        if (a.hiprtcGetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n > 1) {
            log.resize(n);
            a.hiprtcGetProgramLog(prog, &log[0]);
            while (!log.empty() && (log.back() == '\0' || log.back() == '\n')) log.pop_back();
        }
        return fails(job.what + " does not compile: " + a.hiprtcGetErrorString(r) + "\n" + log);
    }
    lowered.clear();
    for (const std::string &e : job.exprs) {
        const char *low = nullptr;
        r = a.hiprtcGetLoweredName(prog, e.c_str(), &low);
        if (r != HIPRTC_SUCCESS || !low) return fails(std::string("hiprtcGetLoweredName: ") + a.hiprtcGetErrorString(r));
        lowered.push_back(low);
    }
    size_t size = 0;
    r = a.hiprtcGetCodeSize(prog, &size);
    if (r == HIPRTC_SUCCESS && size > 0) {
        code.resize(size);
        r = a.hiprtcGetCode(prog, code.data());
    }
    a.hiprtcDestroyProgram(&prog);
    if (r != HIPRTC_SUCCESS || size == 0) { err = std::string("hiprtcGetCode: ") + a.hiprtcGetErrorString(r); return -1; }
    if (const char *dir = getenv("PCL_CELLFN_DUMP")) {     // diagnostics: keep the code object for a disassembler
        const std::string path = std::string(dir) + "/" + job.dump + "_" + std::to_string((*job.dump_seq)++) + ".co";
        if (FILE *fp = fopen(path.c_str(), "wb")) { fwrite(code.data(), 1, code.size(), fp); fclose(fp); }
    }
    return 0;
}

// hiprtc compile of head + preamble + body + tail; math: 0 exact, 1 fast, 2 strict.  0 = ok, else err holds the log
// nout, ops: a functional's outputs (kind PCL_CELLFN_KIND_REDUCE), -D constants like the rest
static inline int cellfn_build(int kind, const char *body, const char *preamble, int meqn, int maux, int ndim, int math,
                               int writes_aux, int reach, std::vector<char> &code, std::string &err, int nout = 0,
                               const int *ops = nullptr) {
    const char *kname = cellfn_kind_label(kind);
    const bool bc = kind == 4, red = kind == PCL_CELLFN_KIND_REDUCE;
    HiprtcJob job;
    job.src = bc ? kCellbcHead : kCellfnHead;
    job.src += "#line 1 \"preamble\"\n";
    job.src += preamble;
    job.src += "\n#line 1 \"pcl_cellfn_wrapper\"\n";
    job.src += bc ? kCellbcOpen : red ? kCellfnReduceOpen : kCellfnOpen;
    job.src += std::string("#line 1 \"") + kname + "\"\n";
    job.src += body;
    job.src += "\n";
    job.src += bc ? kCellbcTail : red ? kCellfnReduceTail : kCellfnTail;
    job.name = "pcl_cellfn.hip";
    // exact / strict: what pclaw.hip itself is built with (no contraction; / and sqrt are IEEE either way)
    job.opts = {"--offload-arch=" PCL_ARCH, "-O3", "-std=c++17", math == 1 ? "-ffp-contract=fast" : "-ffp-contract=off",
                "-DMEQN=" + std::to_string(meqn), "-DMAUX=" + std::to_string(maux), "-DNDIM=" + std::to_string(ndim),
                "-DKIND=" + std::to_string(kind), "-DWRITES_AUX=" + std::to_string(writes_aux ? 1 : 0)};
    if (reach > 0) job.opts.push_back("-DREACH=" + std::to_string(reach));      // reach = 0 passes no -DREACH: the text defaults it
    if (red) {
        std::string list;
        for (int m = 0; m < nout; m++) list += (m ? "," : "") + std::to_string(ops[m]);
        job.opts.push_back("-DNOUT=" + std::to_string(nout));
        job.opts.push_back("-DPCL_OPS=" + list);
    }
    job.what = std::string("cell function (") + kname + ")";
    static int seq = 0;
    job.dump = kname;
    job.dump_seq = &seq;
    std::vector<std::string> none;
    return hiprtc_compile(job, code, none, err);
}

// the modules one solver handle has loaded, by function id; unloaded by pcl_destroy, never by a static destructor
struct CellfnModules {
    struct Loaded { hipModule_t mod; hipFunction_t fn; };
    std::map<long, Loaded> by_id;
    void unload_all() {
        for (auto &kv : by_id) (void)hipModuleUnload(kv.second.mod);
        by_id.clear();
    }
};

}  // namespace pcl
