// Shared helpers for libemp_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/emp_hip.h"

#define EMP_WAVE 64

extern thread_local char emp_err_buf[512];

#define EMP_FAIL(code, ...)                                         \
    do {                                                            \
        snprintf(emp_err_buf, sizeof(emp_err_buf), __VA_ARGS__);    \
        return (code);                                              \
    } while (0)

#define EMP_REQUIRE(cond, ...)                         \
    do {                                               \
        if (!(cond)) EMP_FAIL(EMP_EINVAL, __VA_ARGS__); \
    } while (0)

#define EMP_CHECK_LAUNCH(name)                                                         \
    do {                                                                               \
        hipError_t e_ = hipGetLastError();                                             \
        if (e_ != hipSuccess)                                                          \
            EMP_FAIL(EMP_ELAUNCH, "%s: launch failed: %s", name, hipGetErrorString(e_)); \
    } while (0)

// Launch `kernel` and check the launch under the kernel's own name; returns from the calling function on failure.
// A template kernel goes in parentheses: EMP_LAUNCH((k<4, true>), ...).
#define EMP_LAUNCH(kernel, grid, block, stream, ...)                                      \
    do {                                                                                  \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__);      \
        EMP_CHECK_LAUNCH(#kernel);                                                        \
    } while (0)

static inline hipStream_t emp_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

static inline int64_t emp_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

static inline int64_t emp_align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// Memory-bound grids: cap at 256 CUs x 8 blocks and grid-stride the rest.
static inline int emp_grid(int64_t work_items, int block, int max_blocks = 2048)
{
    int64_t g = emp_cdiv(work_items, block);
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return (int)g;
}

// Workspace carver: hands out typed regions of a caller-provided workspace in call order, each starting at the next
// multiple of `align` bytes, and ends with the total in bytes().  A null base gives null pointers and the same
// total, so one layout function serves both the emp_*_work_bytes query and the entry point: they cannot disagree.
struct EmpCarver {
    char *base;
    int64_t off = 0;
    explicit EmpCarver(void *b) : base(reinterpret_cast<char *>(b)) {}
    template <typename T> T *take(int64_t count, int64_t align = 256)
    {
        off = emp_align_up(off, align);
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += count * (int64_t)sizeof(T);
        return p;
    }
    int64_t bytes() const { return off; }
};

// "Nothing to do": the count is zeroed on the stream and the entry point returns.
static inline int emp_zero_count(int32_t *n_out, hipStream_t st, const char *msg)
{
    if (hipMemsetAsync(n_out, 0, sizeof(int32_t), st) != hipSuccess) EMP_FAIL(EMP_ELAUNCH, "%s", msg);
    return EMP_OK;
}

// Lock-free union-find over int32 parents (parent[i] == i: a root), for the run tables of emp_runs.hip (2D) and
// emp_components.hip (3D).  A unite hangs the LARGER root under the smaller with one atomicMin, so a parent only ever
// decreases, every retry follows a strictly smaller index and the root of a finished set is its smallest member --
// with runs in raster order, the run that holds the component's first voxel.  No thread waits for another.
#ifdef __HIPCC__
__device__ __forceinline__ int uf_find(const int32_t *parent, int a)
{
    int p = parent[a];
    while (p != a) { a = p; p = parent[a]; }
    return a;
}
__device__ __forceinline__ void uf_unite(int32_t *parent, int a, int b)
{
    while (true) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { int t = a; a = b; b = t; }
        int old = atomicMin(&parent[a], b);  // hang the larger root under the smaller
        if (old == a) return;
        a = old;
    }
}

// ------------------------------------------------------------------------------------------ labelled-volume stages
// The labels of the voxels x .. x + 3 of a row as uint32, and the mask of those inside the row.  One aligned load (16
// bytes of uint32, 4 bytes of uint8) where the group lies inside the row on such an address, voxel by voxel otherwise:
// the narrow path, same values.  Positions outside the row read as 0.
template <typename T>
__device__ __forceinline__ uint32_t emp_load4(const T *__restrict__ src, int64_t x, int64_t W, uint32_t *v)
{
    if (x >= 0 && x + 4 <= W && (reinterpret_cast<uintptr_t>(src + x) & (uintptr_t)(4 * sizeof(T) - 1)) == 0) {
        if constexpr (sizeof(T) == 4) {
            const uint4 q = *reinterpret_cast<const uint4 *>(src + x);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            const uint32_t q = *reinterpret_cast<const uint32_t *>(src + x);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (q >> (8 * j)) & 0xffu;
        }
        return 0xfu;
    }
    uint32_t ok = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in = x + j >= 0 && x + j < W;
        v[j] = in ? (uint32_t)src[x + j] : 0u;
        ok |= (uint32_t)in << j;
    }
    return ok;
}
// the same for a row that may be missing: a null row reads as 0
template <typename T>
__device__ __forceinline__ void emp_fetch4(const T *__restrict__ src, int64_t x, int64_t W, uint32_t *v)
{
    if (src == nullptr) v[0] = v[1] = v[2] = v[3] = 0u;
    else emp_load4<T>(src, x, W, v);
}

template <typename T> __global__ void emp_zero_kernel(T *__restrict__ v, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        v[i] = 0;
}

// head[i] = 1 where sorted key i opens a run of keys that are equal above bit SHIFT (0: the whole key; 32: the label
// in the high half)
template <int SHIFT>
__global__ void emp_heads_kernel(const uint64_t *__restrict__ keys, int64_t n, int32_t *__restrict__ head)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        head[i] = (i == 0 || (keys[i - 1] >> SHIFT) != (keys[i] >> SHIFT)) ? 1 : 0;
}

// first index in [lo, hi) whose label (the high half of the key) is >= label (UPPER: > label)
template <bool UPPER>
__device__ __forceinline__ int64_t emp_label_bound(const uint64_t *__restrict__ keys, int64_t lo, int64_t hi, uint64_t label)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t l = keys[mid] >> 32;
        if (UPPER ? l <= label : l < label) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
#endif

// What the entry points that take a label volume (lab, item, D, H, W) ask of it before their own voxel limit and
// alignment; an entry point whose `lab` may be null (D == 0) or is tested later uses EMP_REQUIRE_VOLUME alone.
#define EMP_REQUIRE_VOLUME(what)                                                                                     \
    do {                                                                                                             \
        EMP_REQUIRE(item == 1 || item == 4, what ": labels must be uint8 (1) or uint32 (4), got %d bytes", item);    \
        EMP_REQUIRE(D >= 0 && H > 0 && W > 0, what ": bad shape (D = %lld, H = %lld, W = %lld)", (long long)D,       \
                    (long long)H, (long long)W);                                                                     \
    } while (0)
#define EMP_REQUIRE_LABELS(what)                                                                                     \
    do {                                                                                                             \
        EMP_REQUIRE(lab, what ": null pointer");                                                                     \
        EMP_REQUIRE_VOLUME(what);                                                                                    \
    } while (0)

// The workspace of a "count the rows, then scan" step over R rows: the row counts and the scan's scratch.
struct EmpCountWork {
    int32_t *counts, *scantmp;
    int64_t total;
};
static inline EmpCountWork emp_count_carve(void *work, int64_t R)
{
    if (R < 1) R = 1;
    EmpCarver c(work);
    EmpCountWork L;
    L.counts = c.take<int32_t>(R);
    L.scantmp = c.take<int32_t>(emp_scan_tmp_elems(R));
    L.total = c.bytes();
    return L;
}

// The grid of 8 x 8 x 64 tiles over a slab that the sweeping stages (emp_label_grow.hip, emp_label_thin.hip) work by;
// a slab they accept has at most 2^31 - 1 voxels.
#define EMP_TILE_Z 8
#define EMP_TILE_Y 8
#define EMP_TILE_X 64
struct EmpTiles {
    int64_t nz, ny, nx, n;
};
static inline EmpTiles emp_tiles(int64_t D, int64_t H, int64_t W)
{
    EmpTiles t;
    t.nz = emp_cdiv(D, EMP_TILE_Z);
    t.ny = emp_cdiv(H, EMP_TILE_Y);
    t.nx = emp_cdiv(W, EMP_TILE_X);
    t.n = t.nz * t.ny * t.nx;
    return t;
}
static inline bool emp_tiles_shape_ok(int64_t D, int64_t H, int64_t W)
{
    return D >= 0 && H > 0 && W > 0 && H <= 0x7fffffffLL / W && (D == 0 || H * W <= 0x7fffffffLL / D);
}

// The 26 neighbours of a voxel as one mask (include/emp_hip.h, E8), for emp_label_thin.hip and emp_label_shape.hip:
// position p = 9 (dz + 1) + 3 (dy + 1) + (dx + 1) of the 3 x 3 x 3 block; bit n = p, minus 1 past the centre (p = 13)
static constexpr int lt_pos(int n) { return n < 13 ? n : n + 1; }
static constexpr int lt_abs(int a) { return a < 0 ? -a : a; }
static constexpr int lt_dz(int n) { return lt_pos(n) / 9 - 1; }
static constexpr int lt_dy(int n) { return (lt_pos(n) / 3) % 3 - 1; }
static constexpr int lt_dx(int n) { return lt_pos(n) % 3 - 1; }
#ifdef __HIPCC__
// the label at (z, y, x), z in -1 .. D: the slab, its two neighbour slices where there are any, 0 everywhere else
template <typename T>
__device__ __forceinline__ uint32_t lt_label_at(const T *__restrict__ lab, const T *__restrict__ below,
                                                const T *__restrict__ above, int64_t D, int64_t H, int64_t W, int64_t z,
                                                int64_t y, int64_t x)
{
    if (y < 0 || y >= H || x < 0 || x >= W) return 0;
    if (z >= 0 && z < D) return (uint32_t)lab[(z * H + y) * W + x];
    if (z == -1 && below) return (uint32_t)below[y * W + x];
    if (z == D && above) return (uint32_t)above[y * W + x];
    return 0;
}
#endif

// emp_label_morph.hip: emp_label_edt's three passes with EVERY slice of the extended volume (hb + D + ha slices) as
// output: d2[ze] is the distance inside that volume, whose first and last slices are faces.  d2 and tmp hold one uint16
// per voxel of the extended volume each; the shape must have passed the checks of emp_label_edt_work_bytes.
int emp_label_edt_extended(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below, int64_t hb,
                           const void *above, int64_t ha, int az, int ay, int ax, int cap, uint16_t *d2, uint16_t *tmp,
                           void *stream);

// emp_measure.hip: the run extraction of its rows kernel without the neighbour rows (see there)
int emp_label_rows_extract(const void *lab, int item, int64_t D, int64_t H, int64_t W, const int32_t *row_offsets,
                           int64_t n_runs, int32_t *row, int32_t *xs, int32_t *xe, uint32_t *val, void *stream);

// The run records of an emp_components.hip / emp_holes.hip call, indexed by run (row_offsets[row] + position in the
// row); what the paint step (emp_label_components_paint) reads stays in `work`.  One layout for both files, so that the
// runs of either can be painted.
struct CcWork {
    int32_t *row, *xs, *xe;        // xe: exclusive end
    uint32_t *val;
    int32_t *comp;                 // component index of the run (step 2's second output)
    int32_t *parent, *flag, *pos, *scantmp;
    int64_t keep, total;           // bytes up to and including comp; all of it
};
static inline CcWork cc_carve(void *work, int64_t n)
{
    if (n < 1) n = 1;
    EmpCarver c(work);
    CcWork L;
    L.row = c.take<int32_t>(n);
    L.xs = c.take<int32_t>(n);
    L.xe = c.take<int32_t>(n);
    L.val = c.take<uint32_t>(n);
    L.comp = c.take<int32_t>(n);
    L.keep = c.bytes();
    L.parent = c.take<int32_t>(n);
    L.flag = c.take<int32_t>(n);
    L.pos = c.take<int32_t>(n + 1);
    L.scantmp = c.take<int32_t>(emp_scan_tmp_elems(n));
    L.total = c.bytes();
    return L;
}

// emp_components.hip: the union-find over the runs of L (equal `val`, connectivity 6, 18 or 26) and, after it, the
// flattening that leaves parent[i] = root and flag[i] = (i is a root); one or two launches each
int emp_cc_unite(const CcWork &L, int64_t n_runs, int64_t H, int64_t n_rows, int connectivity,
                 const int32_t *row_offsets, void *stream);
int emp_cc_roots(const CcWork &L, int64_t n_runs, void *stream);

// Stream compaction of n items: launch_flags() fills flag[0..n) with 0/1, the scan turns it into output positions
// pos[0..n] (tmp: emp_scan_tmp_elems(n) elements), launch_emit() writes the flagged items to their positions, and the
// number of them, pos[n], is copied to *n_out.  The two callables launch one kernel each and return EMP_OK or an
// error code.
template <typename Flags, typename Emit>
static inline int emp_compact(const int32_t *flag, int64_t n, int32_t *pos, int32_t *tmp, int32_t *n_out,
                              void *stream, const char *copy_msg, Flags launch_flags, Emit launch_emit)
{
    int rc = launch_flags();
    if (rc != EMP_OK) return rc;
    rc = emp_exclusive_scan_i32(flag, n, pos, tmp, stream);
    if (rc != EMP_OK) return rc;
    rc = launch_emit();
    if (rc != EMP_OK) return rc;
    if (hipMemcpyAsync(n_out, pos + n, sizeof(int32_t), hipMemcpyDeviceToDevice, emp_stream(stream)) != hipSuccess)
        EMP_FAIL(EMP_ELAUNCH, "%s", copy_msg);
    return EMP_OK;
}
