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
#endif

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
