// 3D connected components of a label volume (include/emp_hip.h, E3): one row per component of equal non-zero label
// under 6-, 18- or 26-connectivity, numbered by first voxel in raster order, and the painting of a per-component value
// back over the voxels.  The multi-label rule of cc3d.connected_components, which users of the reference run on a CPU
// after the fact; the definition is the header's.
//
// Count -> scan -> extract as in emp_measure.hip, whose count (emp_label_measure_count) is step 1 here and whose rows
// kernel extracts the runs (emp_label_rows_extract: the centre row alone).  Everything after that is O(#runs): a
// union-find over the runs as in emp_runs.hip's label_union_kernel, with up to four neighbour rows in place of one; the
// roots are numbered by a scan (runs are in raster order and a root is its set's smallest run, so root order IS first
// voxel order); voxels and boxes are integer atomics per run.  No kernel waits on another block.
#include "emp_common.h"

#define CC_COLS 9

extern "C" int64_t emp_label_components_work_bytes(int64_t n_runs) { return cc_carve(nullptr, n_runs).total; }

__global__ void cc_init_kernel(int64_t n, int32_t *__restrict__ parent)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        parent[i] = (int32_t)i;
}

// the runs of row `nr` that run i = [a0, a1) of label v touches, the window widened by w on either side
__device__ __forceinline__ void cc_search(int64_t i, int a0, int a1, uint32_t v, int64_t nr, int w,
                                          const int32_t *__restrict__ xs, const int32_t *__restrict__ xe,
                                          const uint32_t *__restrict__ val, const int32_t *__restrict__ row_offsets,
                                          int32_t *parent)
{
    const int lo = row_offsets[nr], hi = row_offsets[nr + 1];
    int l = lo, h = hi;
    while (l < h) {                                   // first run whose end passes a0 - w
        const int mid = (l + h) >> 1;
        if (xe[mid] > a0 - w) h = mid; else l = mid + 1;
    }
    for (int j = l; j < hi; ++j) {
        if (xs[j] >= a1 + w) break;
        if (val[j] == v) uf_unite(parent, (int)i, j);
    }
}

// Every run looks at the rows before it in raster order: (z, y - 1) and (z - 1, y), which differ on one axis, and for
// 18 / 26 also (z - 1, y - 1) and (z - 1, y + 1), which differ on two.  A step along x on top is one more axis: allowed
// beside a one-axis row from 18 on (w1), beside a two-axis row for 26 alone (w2).
__global__ void cc_union_kernel(int64_t n, int64_t H, int64_t n_rows, int conn, const int32_t *__restrict__ row,
                                const int32_t *__restrict__ xs, const int32_t *__restrict__ xe,
                                const uint32_t *__restrict__ val, const int32_t *__restrict__ row_offsets,
                                int32_t *parent)
{
    const int w1 = conn >= 18 ? 1 : 0, w2 = conn == 26 ? 1 : 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = row[i];
        const int a0 = xs[i], a1 = xe[i];
        if (r < 0 || r >= n_rows || a1 <= a0) continue;
        const uint32_t v = val[i];
        const int64_t z = r / H, y = r - z * H;
        if (y > 0) cc_search(i, a0, a1, v, r - 1, w1, xs, xe, val, row_offsets, parent);
        if (z > 0) {
            cc_search(i, a0, a1, v, r - H, w1, xs, xe, val, row_offsets, parent);
            if (conn >= 18) {
                if (y > 0) cc_search(i, a0, a1, v, r - H - 1, w2, xs, xe, val, row_offsets, parent);
                if (y + 1 < H) cc_search(i, a0, a1, v, r - H + 1, w2, xs, xe, val, row_offsets, parent);
            }
        }
    }
}

__global__ void cc_flatten_kernel(int64_t n, int32_t *parent, int32_t *__restrict__ flag)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = uf_find(parent, (int)i);
        flag[i] = (r == (int)i) ? 1 : 0;
        // roots do not change any more, so writing the root is race-free with the finds of other threads
        if (r != (int)i) parent[i] = r;
    }
}

// the two halves of the union-find as launches, for this file and for emp_holes.hip (whose runs all carry value 0)
int emp_cc_unite(const CcWork &L, int64_t n_runs, int64_t H, int64_t n_rows, int connectivity,
                 const int32_t *row_offsets, void *stream)
{
    hipStream_t st = emp_stream(stream);
    const int grid = emp_grid(n_runs, 256, 4096);
    EMP_LAUNCH(cc_init_kernel, grid, 256, st, n_runs, L.parent);
    EMP_LAUNCH(cc_union_kernel, grid, 256, st, n_runs, H, n_rows, connectivity, L.row, L.xs, L.xe, L.val, row_offsets,
               L.parent);
    return EMP_OK;
}

int emp_cc_roots(const CcWork &L, int64_t n_runs, void *stream)
{
    EMP_LAUNCH(cc_flatten_kernel, emp_grid(n_runs, 256, 4096), 256, emp_stream(stream), n_runs, L.parent, L.flag);
    return EMP_OK;
}

// pos[root] numbers the roots in run order; the root's own thread starts the component's row
__global__ void cc_comp_kernel(int64_t n, int64_t W, int64_t first_base, const int32_t *__restrict__ parent,
                               const int32_t *__restrict__ flag, const int32_t *__restrict__ pos,
                               const int32_t *__restrict__ row, const int32_t *__restrict__ xs,
                               const uint32_t *__restrict__ val, int32_t *__restrict__ comp,
                               int64_t *__restrict__ table)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = pos[parent[i]];
        comp[i] = k;
        if (flag[i]) {
            int64_t *t = table + (int64_t)k * CC_COLS;
            t[0] = (int64_t)val[i];
            t[1] = 0;
            t[2] = first_base + (int64_t)row[i] * W + xs[i];
            t[3] = t[4] = t[5] = 0x7fffffffffffffffLL;
            t[6] = t[7] = t[8] = 0;
        }
    }
}

// integer add / min / max per run: neither the order of the atomics nor the launch shape shows
__global__ void cc_stats_kernel(int64_t n, int64_t H, int64_t z_base, const int32_t *__restrict__ row,
                                const int32_t *__restrict__ xs, const int32_t *__restrict__ xe,
                                const int32_t *__restrict__ comp, int64_t *__restrict__ table)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = row[i];
        const int64_t zl = r / H, y = r - zl * H, z = zl + z_base;
        const int64_t x0 = xs[i], x1 = xe[i];
        if (x1 <= x0) continue;
        unsigned long long *t = reinterpret_cast<unsigned long long *>(table + (int64_t)comp[i] * CC_COLS);
        atomicAdd(t + 1, (unsigned long long)(x1 - x0));
        // a minimum only falls and a maximum only rises, so a value read earlier is never better than the current one:
        // a run that cannot improve on what it reads cannot improve on the row either, and most runs lie inside the box
        if ((unsigned long long)z < t[3]) atomicMin(t + 3, (unsigned long long)z);
        if ((unsigned long long)y < t[4]) atomicMin(t + 4, (unsigned long long)y);
        if ((unsigned long long)x0 < t[5]) atomicMin(t + 5, (unsigned long long)x0);
        if ((unsigned long long)(z + 1) > t[6]) atomicMax(t + 6, (unsigned long long)(z + 1));
        if ((unsigned long long)(y + 1) > t[7]) atomicMax(t + 7, (unsigned long long)(y + 1));
        if ((unsigned long long)x1 > t[8]) atomicMax(t + 8, (unsigned long long)x1);
    }
}

// same shape checks as emp_measure.hip: one run per voxel is the worst case and the scan is int32
#define CC_REQUIRE_SHAPE(what)                                                                                       \
    do {                                                                                                             \
        EMP_REQUIRE_LABELS(what);                                                                                    \
        EMP_REQUIRE(H <= 0x7fffffffLL / W && (D == 0 || H * W <= 0x7fffffffLL / D),                                  \
                    what ": %lld x %lld x %lld voxels could hold more than 2^31 - 1 runs; cut the slab into z-blocks", \
                    (long long)D, (long long)H, (long long)W);                                                       \
        EMP_REQUIRE((reinterpret_cast<uintptr_t>(lab) % (uintptr_t)item) == 0, what ": misaligned labels");          \
    } while (0)

extern "C" int emp_label_components(const void *lab, int item, int64_t D, int64_t H, int64_t W, int connectivity,
                                    int64_t z_base, const int32_t *row_offsets, int64_t n_runs, void *work,
                                    int64_t work_bytes, int64_t *out_table, int32_t *n_out, void *stream)
{
    CC_REQUIRE_SHAPE("label_components");
    EMP_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26,
                "label_components: connectivity must be 6, 18 or 26, got %d", connectivity);
    EMP_REQUIRE(row_offsets && n_out, "label_components: null pointer");
    EMP_REQUIRE(z_base >= 0 && z_base <= (1LL << 40), "label_components: z_base = %lld outside 0 .. 2^40",
                (long long)z_base);
    EMP_REQUIRE(n_runs >= 0 && n_runs <= D * H * W,
                "label_components: n_runs = %lld is not the run total of %lld voxels", (long long)n_runs,
                (long long)(D * H * W));
    hipStream_t st = emp_stream(stream);
    if (n_runs == 0) return emp_zero_count(n_out, st, "label_components: memset");
    EMP_REQUIRE(work && out_table, "label_components: null pointer");
    CcWork L = cc_carve(work, n_runs);
    EMP_REQUIRE(work_bytes >= L.total, "label_components: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.total);
    // a slot that the extraction does not reach (labels changed since step 1) reads as an empty run of row 0
    if (hipMemsetAsync(L.row, 0, (size_t)L.keep, st) != hipSuccess) EMP_FAIL(EMP_ELAUNCH, "label_components: memset");
    int rc = emp_label_rows_extract(lab, item, D, H, W, row_offsets, n_runs, L.row, L.xs, L.xe, L.val, stream);
    if (rc != EMP_OK) return rc;
    const int grid = emp_grid(n_runs, 256, 4096);
    rc = emp_cc_unite(L, n_runs, H, D * H, connectivity, row_offsets, stream);
    if (rc != EMP_OK) return rc;
    rc = emp_compact(
        L.flag, n_runs, L.pos, L.scantmp, n_out, stream, "label_components: count copy",
        [&]() -> int { return emp_cc_roots(L, n_runs, stream); },
        [&]() -> int {
            EMP_LAUNCH(cc_comp_kernel, grid, 256, st, n_runs, W, z_base * H * W, L.parent, L.flag, L.pos, L.row, L.xs,
                       L.val, L.comp, out_table);
            return EMP_OK;
        });
    if (rc != EMP_OK) return rc;
    EMP_LAUNCH(cc_stats_kernel, grid, 256, st, n_runs, H, z_base, L.row, L.xs, L.xe, L.comp, out_table);
    return EMP_OK;
}

// ------------------------------------------------------------------------------------------ paint
// 16 lanes per run.  A run starts anywhere, so its head up to the next 16-byte address and its tail go out element by
// element and the groups between as 16-byte stores: the same bytes either way.  In place (skip_same) a run whose value
// stays is not written at all, so a repair costs the runs it changes.
template <typename T>
__global__ __launch_bounds__(256) void cc_paint_kernel(int64_t n_runs, int64_t H, int64_t W, int64_t n_comp, int64_t z_lo,
                                                       int64_t z_hi, const int32_t *__restrict__ row_offsets,
                                                       const int32_t *__restrict__ row, const int32_t *__restrict__ xs,
                                                       const int32_t *__restrict__ xe, const uint32_t *__restrict__ val,
                                                       const int32_t *__restrict__ comp, const uint32_t *__restrict__ lut,
                                                       int skip_same, T *__restrict__ dst)
{
    constexpr int VE = 16 / (int)sizeof(T);           // elements of one vector store
    const int sub = threadIdx.x & 15;
    const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int64_t n_groups = ((int64_t)gridDim.x * blockDim.x) >> 4;
    int64_t r_lo = row_offsets[z_lo * H], r_hi = row_offsets[z_hi * H];
    if (r_hi > n_runs) r_hi = n_runs;
    for (int64_t i = r_lo + group; i < r_hi; i += n_groups) {
        const int64_t r = row[i], x0 = xs[i], x1 = xe[i];
        const int64_t k = comp[i];
        if (r < z_lo * H || r >= z_hi * H || x0 < 0 || x1 > W || x1 <= x0 || k < 0 || k >= n_comp) continue;
        const uint32_t v = lut[k];
        if (skip_same && v == val[i]) continue;
        T *p = dst + ((r - z_lo * H) * W + x0);
        const int64_t len = x1 - x0;
        const int mis = (int)((reinterpret_cast<uintptr_t>(p) / sizeof(T)) & (uintptr_t)(VE - 1));
        int64_t head = (VE - mis) & (VE - 1);
        if (head > len) head = len;
        const int64_t body = (len - head) / VE, tail = len - head - body * VE;
        for (int64_t e = sub; e < head; e += 16) p[e] = (T)v;
        uint4 q;
        if constexpr (sizeof(T) == 4) q.x = v; else q.x = (v & 0xffu) * 0x01010101u;
        q.y = q.z = q.w = q.x;
        uint4 *pv = reinterpret_cast<uint4 *>(p + head);
        for (int64_t g = sub; g < body; g += 16) pv[g] = q;
        T *pt = p + head + body * VE;
        for (int64_t e = sub; e < tail; e += 16) pt[e] = (T)v;
    }
}

extern "C" int emp_label_components_paint(const void *lab, int item, int64_t D, int64_t H, int64_t W,
                                          const int32_t *row_offsets, int64_t n_runs, const void *work,
                                          int64_t work_bytes, const uint32_t *lut, int64_t n_comp, int64_t z_lo,
                                          int64_t z_hi, void *dst, int dst_item, void *stream)
{
    CC_REQUIRE_SHAPE("label_components_paint");
    EMP_REQUIRE(row_offsets, "label_components_paint: null pointer");
    EMP_REQUIRE(dst_item == 1 || dst_item == 4, "label_components_paint: dst must be uint8 (1) or uint32 (4), got %d bytes",
                dst_item);
    EMP_REQUIRE(0 <= z_lo && z_lo <= z_hi && z_hi <= D, "label_components_paint: slices [%lld, %lld) outside 0 .. %lld",
                (long long)z_lo, (long long)z_hi, (long long)D);
    EMP_REQUIRE(n_runs >= 0 && n_runs <= D * H * W && n_comp >= 0 && n_comp <= n_runs,
                "label_components_paint: n_runs = %lld, n_comp = %lld are not those of step 2", (long long)n_runs,
                (long long)n_comp);
    if (z_lo == z_hi) return EMP_OK;
    EMP_REQUIRE(dst && reinterpret_cast<uintptr_t>(dst) % (uintptr_t)dst_item == 0,
                "label_components_paint: null or misaligned dst");
    const int64_t slice = H * W;
    const char *src_lo = reinterpret_cast<const char *>(lab) + z_lo * slice * item;
    const char *lab_end = reinterpret_cast<const char *>(lab) + D * slice * item;
    const char *d0 = reinterpret_cast<const char *>(dst), *d1 = d0 + (z_hi - z_lo) * slice * dst_item;
    const bool in_place = d0 == src_lo && dst_item == item;
    EMP_REQUIRE(in_place || d1 <= reinterpret_cast<const char *>(lab) || d0 >= lab_end,
                "label_components_paint: dst overlaps the labels without being their slices [z_lo, z_hi) themselves");
    hipStream_t st = emp_stream(stream);
    if (!in_place && hipMemsetAsync(dst, 0, (size_t)(d1 - d0), st) != hipSuccess)
        EMP_FAIL(EMP_ELAUNCH, "label_components_paint: memset");
    if (n_runs == 0) return EMP_OK;
    EMP_REQUIRE(work && lut, "label_components_paint: null pointer");
    CcWork L = cc_carve(const_cast<void *>(work), n_runs);
    EMP_REQUIRE(work_bytes >= L.keep, "label_components_paint: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.keep);
    const int grid = emp_grid(n_runs * 16, 256, 8192);
    if (dst_item == 4)
        EMP_LAUNCH((cc_paint_kernel<uint32_t>), grid, 256, st, n_runs, H, W, n_comp, z_lo, z_hi, row_offsets, L.row, L.xs,
                   L.xe, L.val, L.comp, lut, in_place ? 1 : 0, reinterpret_cast<uint32_t *>(dst));
    else
        EMP_LAUNCH((cc_paint_kernel<uint8_t>), grid, 256, st, n_runs, H, W, n_comp, z_lo, z_hi, row_offsets, L.row, L.xs,
                   L.xe, L.val, L.comp, lut, in_place ? 1 : 0, reinterpret_cast<uint8_t *>(dst));
    return EMP_OK;
}
