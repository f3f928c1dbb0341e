// T1 on the device: run tables of a plane's slices -> per-instance 3D run lists, sorted by (instance, start),
// without leaving HBM.  replaces InstanceTracker.update / finish (empanada/inference/tracker.py:61-123) for the
// whole-stack path; the consensus (C1/C3/C4) and the fill (Z1) consume these arrays directly.
//
// A 3D run is (key, len): key = instance << 40 | flat (z, y, x) start, len in voxels.  40 bits of start cover
// 2^40 voxels (cfg 5 has 2^32), 24 bits of instance 16.7 M instances per plane set.
#include "emp_common.h"

#define TRK_POS_BITS 40
#define TRK_POS_MASK ((1ULL << TRK_POS_BITS) - 1ULL)

// ------------------------------------------------------------------------------------------ xy / xz lift
// Run i continues run i-1 (same instance, same slice, flat 2D indices contiguous) exactly when rle_encode over the
// instance's pixels of that slice would not start a new run there (array_utils.py:209-235): the table is in raster
// order, so the only run that can end at start-1 is the previous one.
__device__ __forceinline__ bool trk_continues(const int32_t *r_start, const int32_t *r_len, const int32_t *r_comp,
                                              const int32_t *c_slice, const int32_t *comp_inst, int64_t i)
{
    if (i == 0) return false;
    int ca = r_comp[i - 1], cb = r_comp[i];
    int ia = comp_inst[ca], ib = comp_inst[cb];
    return ib >= 0 && ia == ib && c_slice[ca] == c_slice[cb] && r_start[i - 1] + r_len[i - 1] == r_start[i];
}

__global__ void trk_heads_kernel(const int32_t *__restrict__ r_start, const int32_t *__restrict__ r_len,
                                 const int32_t *__restrict__ r_comp, const int32_t *__restrict__ c_slice,
                                 const int32_t *__restrict__ comp_inst, int64_t n, int32_t *__restrict__ head)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        head[i] = (comp_inst[r_comp[i]] >= 0 && !trk_continues(r_start, r_len, r_comp, c_slice, comp_inst, i)) ? 1 : 0;
}

__global__ void trk_emit_kernel(int axis, const int32_t *__restrict__ r_start, const int32_t *__restrict__ r_len,
                                const int32_t *__restrict__ r_comp, const int32_t *__restrict__ c_slice,
                                const int32_t *__restrict__ comp_inst, int64_t n, int W, int64_t YX, int X,
                                int slice0, int64_t inst_base, int64_t origin, const int32_t *__restrict__ head,
                                const int32_t *__restrict__ pos, uint64_t *__restrict__ out_key,
                                int64_t *__restrict__ out_len)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (!head[i]) continue;
        int comp = r_comp[i];
        int64_t len = r_len[i];
        for (int64_t j = i + 1; j < n && trk_continues(r_start, r_len, r_comp, c_slice, comp_inst, j); ++j)
            len += r_len[j];
        int64_t st = r_start[i];
        int64_t sl = (int64_t)c_slice[comp] + slice0;
        int64_t st3;
        if (axis == 0) st3 = st + sl * YX;                                   // plane (Y, X), slices along z
        else if (axis == 1) st3 = (st / W) * YX + sl * (int64_t)X + (st % W);   // plane (Z, X), slices along y: only the
                                                                             // START is mapped (tracker.py:78-82)
        else st3 = (st / W) * (int64_t)X + (st % W) + origin;                // tile (., W) inside an image (., X): 2D
                                                                             // start, length kept (tile.py:155-166)
        int64_t o = pos[i];
        out_key[o] = ((uint64_t)(inst_base + comp_inst[comp]) << TRK_POS_BITS) | (uint64_t)st3;
        out_len[o] = len;
    }
}

extern "C" int64_t emp_track_work_elems(int64_t n_runs)
{
    int64_t n = n_runs > 0 ? n_runs : 1;
    return 2 * n + 2 + emp_scan_tmp_elems(n);
}

// heads -> scan -> emit over a run table, shared by emp_track_lift (axis 0 / 1) and emp_tile_lift (axis 2)
static int trk_lift(int axis, const int32_t *r_start, const int32_t *r_len, const int32_t *r_comp,
                    const int32_t *c_slice, const int32_t *comp_inst, int64_t n_runs, int W, int64_t YX, int X,
                    int slice0, int64_t inst_base, int64_t origin, int32_t *work, uint64_t *out_key,
                    int64_t *out_len, int32_t *n_out, void *stream, const char *copy_msg)
{
    hipStream_t st = emp_stream(stream);
    int32_t *head = work, *pos = work + n_runs, *tmp = work + 2 * n_runs + 2;
    int grid = emp_grid(n_runs, 256, 4096);
    return emp_compact(
        head, n_runs, pos, tmp, n_out, stream, copy_msg,
        [&]() -> int {
            EMP_LAUNCH(trk_heads_kernel, grid, 256, st, r_start, r_len, r_comp, c_slice, comp_inst, n_runs, head);
            return EMP_OK;
        },
        [&]() -> int {
            EMP_LAUNCH(trk_emit_kernel, grid, 256, st, axis, r_start, r_len, r_comp, c_slice, comp_inst, n_runs, W, YX,
                       X, slice0, inst_base, origin, head, pos, out_key, out_len);
            return EMP_OK;
        });
}

extern "C" int emp_track_lift(int axis, const int32_t *r_start, const int32_t *r_len, const int32_t *r_comp,
                              const int32_t *c_slice, const int32_t *comp_inst, int64_t n_runs, int H, int W, int Y,
                              int X, int slice0, int64_t inst_base, int32_t *work, uint64_t *out_key,
                              int64_t *out_len, int32_t *n_out, void *stream)
{
    EMP_REQUIRE(axis == 0 || axis == 1, "track_lift: axis must be 0 (xy) or 1 (xz); yz goes through emp_track_lift_yz");
    EMP_REQUIRE(n_runs >= 0 && n_runs < (1LL << 31) && H > 0 && W > 0 && Y > 0 && X > 0 && slice0 >= 0 && n_out,
                "track_lift: bad sizes");
    EMP_REQUIRE(axis == 0 ? (H == Y && W == X) : (W == X), "track_lift: plane shape does not match the volume");
    if (n_runs == 0) return emp_zero_count(n_out, emp_stream(stream), "track_lift: memset");
    EMP_REQUIRE(r_start && r_len && r_comp && c_slice && comp_inst && work && out_key && out_len,
                "track_lift: null pointer");
    return trk_lift(axis, r_start, r_len, r_comp, c_slice, comp_inst, n_runs, W, (int64_t)Y * X, X, slice0, inst_base,
                    0, work, out_key, out_len, n_out, stream, "track_lift: count copy");
}

// ------------------------------------------------------------------------------------------ tile lift (C5)
// Tiler.translate_rle_seg (empanada/inference/tile.py:122-168) for a whole stack of one tile's slices: the runs of
// every object (component of the tile's run table) merged where rle_encode of its flat TILE indices would merge them
// (a run ending at the tile's last column continues at column 0 of the next row, array_utils.py:209-235), the START
// mapped into the image frame -- (start / tw + y0) * X + start % tw + x0 -- and the length kept, so a run that wrapped
// inside the tile runs on past the tile's right edge in the image, exactly as in the reference.  Positions are 2D
// (the slice is carried by the object): key = (inst_base + comp_inst[comp]) << 40 | start2d.
extern "C" int emp_tile_lift(const int32_t *r_start, const int32_t *r_len, const int32_t *r_comp,
                             const int32_t *c_slice, const int32_t *comp_inst, int64_t n_runs, int tw, int X, int y0,
                             int x0, int64_t inst_base, int32_t *work, uint64_t *out_key, int64_t *out_len,
                             int32_t *n_out, void *stream)
{
    EMP_REQUIRE(n_runs >= 0 && n_runs < (1LL << 31) && tw > 0 && X >= tw && y0 >= 0 && x0 >= 0 && x0 + tw <= X && n_out,
                "tile_lift: bad sizes");
    if (n_runs == 0) return emp_zero_count(n_out, emp_stream(stream), "tile_lift: memset");
    EMP_REQUIRE(r_start && r_len && r_comp && c_slice && comp_inst && work && out_key && out_len,
                "tile_lift: null pointer");
    return trk_lift(2, r_start, r_len, r_comp, c_slice, comp_inst, n_runs, tw, 0, X, 0, inst_base,
                    (int64_t)y0 * X + x0, work, out_key, out_len, n_out, stream, "tile_lift: count copy");
}

// ------------------------------------------------------------------------------------------ yz lift
// The yz tracker is the run-length encoding along x of the dense labelling (tracker.py:83-88,110-113): the runs of
// the scattered (Z, Y, Xl) volume (emp_scatter_yz_u32 with value = instance + 1, then emp_runs_count / _extract)
// are already that encoding; this kernel only turns (row, x) into flat starts of the full (Z, Y, X) frame.
__global__ void trk_yz_kernel(const int32_t *__restrict__ row_offsets, const int32_t *__restrict__ r_start,
                              const int32_t *__restrict__ r_len, const uint32_t *__restrict__ r_val, int64_t n_rows,
                              int64_t n, int Xl, int X, int x0, int64_t inst_base, uint64_t *__restrict__ out_key,
                              int64_t *__restrict__ out_len)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = n_rows;                         // last row whose offset is <= i
        while (hi - lo > 1) {
            int64_t mid = (lo + hi) >> 1;
            if ((int64_t)row_offsets[mid] <= i) lo = mid; else hi = mid;
        }
        int64_t st3 = lo * (int64_t)X + x0 + (r_start[i] % Xl);
        out_key[i] = ((uint64_t)(inst_base + (int64_t)r_val[i] - 1) << TRK_POS_BITS) | (uint64_t)st3;
        out_len[i] = r_len[i];
    }
}

extern "C" int emp_track_lift_yz(const int32_t *row_offsets, const int32_t *r_start, const int32_t *r_len,
                                 const uint32_t *r_val, int64_t n_rows, int64_t n_runs, int Xl, int X, int x0,
                                 int64_t inst_base, uint64_t *out_key, int64_t *out_len, void *stream)
{
    EMP_REQUIRE(n_runs >= 0 && n_rows > 0 && Xl > 0 && X >= Xl && x0 >= 0 && x0 + Xl <= X, "track_lift_yz: bad sizes");
    if (n_runs == 0) return EMP_OK;
    EMP_REQUIRE(row_offsets && r_start && r_len && r_val && out_key && out_len, "track_lift_yz: null pointer");
    EMP_LAUNCH(trk_yz_kernel, emp_grid(n_runs, 256, 4096), 256, emp_stream(stream), row_offsets, r_start, r_len, r_val,
               n_rows, n_runs, Xl, X, x0, inst_base, out_key, out_len);
    return EMP_OK;
}

// ------------------------------------------------------------------------------------------ sort (+ merge)
struct TrkSortWork {
    uint64_t *keys;
    int32_t *idx_in, *idx_out;
    int64_t *len;
    int32_t *flag, *pos, *scantmp;
    char *cub;
    int64_t cub_bytes, total;
};
// work == nullptr: only .total (and .cub_bytes) mean anything -- the size query
static TrkSortWork trk_sort_carve(void *work, int64_t n)
{
    if (n < 1) n = 1;
    EmpCarver c(work);
    TrkSortWork L;
    L.keys = c.take<uint64_t>(n);
    L.idx_in = c.take<int32_t>(n);
    L.idx_out = c.take<int32_t>(n);
    L.len = c.take<int64_t>(n);
    L.flag = c.take<int32_t>(n);
    L.pos = c.take<int32_t>(n + 1);
    L.scantmp = c.take<int32_t>(emp_scan_tmp_elems(n));
    L.cub_bytes = emp_sort_work_bytes(n);
    L.cub = c.take<char>(L.cub_bytes);
    L.total = c.bytes();
    return L;
}
extern "C" int64_t emp_track_sort_work_bytes(int64_t n) { return trk_sort_carve(nullptr, n).total; }

__global__ void trk_set_kernel(int32_t *p, int32_t v) { *p = v; }

__global__ void trk_iota_kernel(int32_t *__restrict__ v, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        v[i] = (int32_t)i;
}

__global__ void trk_gather_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ idx,
                                  const int64_t *__restrict__ len_in, int64_t n, uint64_t *__restrict__ out_key,
                                  int64_t *__restrict__ out_st, int64_t *__restrict__ out_len)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t k = keys[i];
        if (out_key) out_key[i] = k;
        if (out_st) out_st[i] = (int64_t)(k & TRK_POS_MASK);
        out_len[i] = len_in[idx[i]];
    }
}

// runs of one instance that touch (previous end == start) become one run: np.sort + rle_encode of tracker.finish
__global__ void trk_touch_heads_kernel(const uint64_t *__restrict__ keys, const int64_t *__restrict__ len, int64_t n,
                                       int32_t *__restrict__ head)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        head[i] = (i == 0 || keys[i - 1] + (uint64_t)len[i - 1] != keys[i]) ? 1 : 0;   // a carry into the instance
                                                                                       // bits cannot equal keys[i]
}

__global__ void trk_touch_emit_kernel(const uint64_t *__restrict__ keys, const int64_t *__restrict__ len, int64_t n,
                                      const int32_t *__restrict__ head, const int32_t *__restrict__ pos,
                                      uint64_t *__restrict__ out_key, int64_t *__restrict__ out_st,
                                      int64_t *__restrict__ out_len)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (!head[i]) continue;
        int64_t total = len[i];
        for (int64_t j = i + 1; j < n && !head[j]; ++j) total += len[j];
        int64_t o = pos[i];
        if (out_key) out_key[o] = keys[i];
        if (out_st) out_st[o] = (int64_t)(keys[i] & TRK_POS_MASK);
        out_len[o] = total;
    }
}

extern "C" int emp_track_sort(const uint64_t *key_in, const int64_t *len_in, int64_t n, int merge_touching,
                              void *work, int64_t work_bytes, uint64_t *out_key, int64_t *out_st, int64_t *out_len,
                              int32_t *n_out, void *stream)
{
    EMP_REQUIRE(n >= 0 && n < (1LL << 31) && n_out, "track_sort: bad arguments");
    hipStream_t st = emp_stream(stream);
    if (n == 0) return emp_zero_count(n_out, st, "track_sort: memset");
    EMP_REQUIRE(key_in && len_in && work && out_len, "track_sort: null pointer");
    TrkSortWork L = trk_sort_carve(work, n);
    EMP_REQUIRE(work_bytes >= L.total, "track_sort: workspace too small");
    int grid = emp_grid(n, 256, 4096);
    EMP_LAUNCH(trk_iota_kernel, grid, 256, st, L.idx_in, n);
    int rc = emp_sort_u64_i32(key_in, L.keys, L.idx_in, L.idx_out, n, 0, 64, L.cub, L.cub_bytes, stream);
    if (rc != EMP_OK) return rc;
    if (!merge_touching) {
        EMP_LAUNCH(trk_gather_kernel, grid, 256, st, L.keys, L.idx_out, len_in, n, out_key, out_st, out_len);
        EMP_LAUNCH(trk_set_kernel, 1, 1, st, n_out, (int32_t)n);
        return EMP_OK;
    }
    EMP_LAUNCH(trk_gather_kernel, grid, 256, st, L.keys, L.idx_out, len_in, n, (uint64_t *)nullptr, (int64_t *)nullptr,
               L.len);
    return emp_compact(
        L.flag, n, L.pos, L.scantmp, n_out, stream, "track_sort: count copy",
        [&]() -> int {
            EMP_LAUNCH(trk_touch_heads_kernel, grid, 256, st, L.keys, L.len, n, L.flag);
            return EMP_OK;
        },
        [&]() -> int {
            EMP_LAUNCH(trk_touch_emit_kernel, grid, 256, st, L.keys, L.len, n, L.flag, L.pos, out_key, out_st, out_len);
            return EMP_OK;
        });
}

// ------------------------------------------------------------------------------------------ small table kernels
// out_off[k] = first sorted run whose instance is >= k, k = 0 .. n_inst (CSR offsets of the instances)
__global__ void trk_offsets_kernel(const uint64_t *__restrict__ keys, int64_t n, int64_t n_inst,
                                   int64_t *__restrict__ out_off)
{
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n_inst) return;
    uint64_t key = (uint64_t)k << TRK_POS_BITS;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    out_off[k] = lo;
}

extern "C" int emp_track_offsets(const uint64_t *keys_sorted, int64_t n, int64_t n_inst, int64_t *out_off,
                                 void *stream)
{
    EMP_REQUIRE(n >= 0 && n_inst >= 0 && n_inst < (1LL << 24) && out_off, "track_offsets: bad arguments");
    EMP_REQUIRE(n == 0 || keys_sorted, "track_offsets: null keys");
    EMP_LAUNCH(trk_offsets_kernel, (unsigned)emp_cdiv(n_inst + 1, 256), 256, emp_stream(stream), keys_sorted, n, n_inst,
               out_off);
    return EMP_OK;
}

// out[i] = obj_val[instance of run i] for runs stored instance by instance (off = CSR offsets over n_obj instances)
__global__ void trk_expand_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ obj_val, int64_t n_obj,
                                  int64_t n, int32_t *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = n_obj;                          // last instance whose offset is <= i
        while (hi - lo > 1) {
            int64_t mid = (lo + hi) >> 1;
            if (off[mid] <= i) lo = mid; else hi = mid;
        }
        out[i] = obj_val[lo];
    }
}

extern "C" int emp_track_expand(const int64_t *off, const int32_t *obj_val, int64_t n_obj, int64_t n_runs,
                                int32_t *out, void *stream)
{
    EMP_REQUIRE(n_obj > 0 && n_runs >= 0, "track_expand: bad sizes");
    if (n_runs == 0) return EMP_OK;
    EMP_REQUIRE(off && obj_val && out, "track_expand: null pointer");
    EMP_LAUNCH(trk_expand_kernel, emp_grid(n_runs, 256, 4096), 256, emp_stream(stream), off, obj_val, n_obj, n_runs, out);
    return EMP_OK;
}

// keep the part of every run that lies in the flat voxel interval [lo, hi) (a rank's z-slab of the output volume;
// zarr_utils.py:11-47 splits runs at chunk borders the same way)
__global__ void trk_clip_flags_kernel(const uint64_t *__restrict__ key, const int64_t *__restrict__ len, int64_t n,
                                      int64_t lo, int64_t hi, int32_t *__restrict__ keep)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t s = (int64_t)(key[i] & TRK_POS_MASK), e = s + len[i];
        keep[i] = ((s > lo ? s : lo) < (e < hi ? e : hi)) ? 1 : 0;
    }
}

__global__ void trk_clip_emit_kernel(const uint64_t *__restrict__ key, const int64_t *__restrict__ len, int64_t n,
                                     int64_t lo, int64_t hi, const int32_t *__restrict__ keep,
                                     const int32_t *__restrict__ pos, uint64_t *__restrict__ out_key,
                                     int64_t *__restrict__ out_len)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (!keep[i]) continue;
        int64_t s = (int64_t)(key[i] & TRK_POS_MASK), e = s + len[i];
        int64_t s2 = s > lo ? s : lo, e2 = e < hi ? e : hi;
        int64_t o = pos[i];
        out_key[o] = (key[i] & ~TRK_POS_MASK) | (uint64_t)s2;
        out_len[o] = e2 - s2;
    }
}

extern "C" int emp_track_clip(const uint64_t *key, const int64_t *len, int64_t n, int64_t lo, int64_t hi,
                              int32_t *work, uint64_t *out_key, int64_t *out_len, int32_t *n_out, void *stream)
{
    EMP_REQUIRE(n >= 0 && n < (1LL << 31) && lo >= 0 && hi >= lo && n_out, "track_clip: bad arguments");
    hipStream_t st = emp_stream(stream);
    if (n == 0) return emp_zero_count(n_out, st, "track_clip: memset");
    EMP_REQUIRE(key && len && work && out_key && out_len, "track_clip: null pointer");
    int32_t *keep = work, *pos = work + n, *tmp = work + 2 * n + 2;
    int grid = emp_grid(n, 256, 4096);
    return emp_compact(
        keep, n, pos, tmp, n_out, stream, "track_clip: count copy",
        [&]() -> int {
            EMP_LAUNCH(trk_clip_flags_kernel, grid, 256, st, key, len, n, lo, hi, keep);
            return EMP_OK;
        },
        [&]() -> int {
            EMP_LAUNCH(trk_clip_emit_kernel, grid, 256, st, key, len, n, lo, hi, keep, pos, out_key, out_len);
            return EMP_OK;
        });
}

// ------------------------------------------------------------------------------------------ overlap triplets
// emp_runs_overlap_next emits one (comp_a, comp_b, pixels) triplet per overlapping RUN pair (~20 per component pair at
// 1024^2); the chain wants one per COMPONENT pair.  Sort by (a, b) and sum the equal keys on the device, so that the
// host receives and walks O(#component pairs) entries instead of O(#run pairs).
__global__ void trip_keys_kernel(const int32_t *__restrict__ trip, int64_t n, uint64_t *__restrict__ keys,
                                 int32_t *__restrict__ vals)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        keys[i] = ((uint64_t)(uint32_t)trip[3 * i] << 32) | (uint64_t)(uint32_t)trip[3 * i + 1];
        vals[i] = trip[3 * i + 2];
    }
}

__global__ void trip_emit_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ vals, int64_t n,
                                 const int32_t *__restrict__ head, const int32_t *__restrict__ pos,
                                 int32_t *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (!head[i]) continue;
        int32_t total = vals[i];
        for (int64_t j = i + 1; j < n && !head[j]; ++j) total += vals[j];
        const int64_t o = pos[i];
        out[3 * o] = (int32_t)(keys[i] >> 32);
        out[3 * o + 1] = (int32_t)(keys[i] & 0xffffffffULL);
        out[3 * o + 2] = total;
    }
}

struct TripWork {
    uint64_t *keys_in, *keys_out;
    int32_t *vals_in, *vals_out, *head, *pos, *scantmp;
    char *cub;
    int64_t cub_bytes, total;
};
static TripWork trip_carve(void *work, int64_t n)
{
    if (n < 1) n = 1;
    EmpCarver c(work);
    TripWork L;
    L.keys_in = c.take<uint64_t>(n);
    L.keys_out = c.take<uint64_t>(n);
    L.vals_in = c.take<int32_t>(n);
    L.vals_out = c.take<int32_t>(n);
    L.head = c.take<int32_t>(n);
    L.pos = c.take<int32_t>(n + 1);
    L.scantmp = c.take<int32_t>(emp_scan_tmp_elems(n));
    L.cub_bytes = emp_sort_work_bytes(n);
    L.cub = c.take<char>(L.cub_bytes);
    L.total = c.bytes();
    return L;
}
extern "C" int64_t emp_triplets_reduce_work_bytes(int64_t n) { return trip_carve(nullptr, n).total; }

extern "C" int emp_triplets_reduce(const int32_t *trip, int64_t n, void *work, int64_t work_bytes, int32_t *out,
                                   int32_t *n_out, void *stream)
{
    EMP_REQUIRE(n >= 0 && n < (1LL << 31) && n_out, "triplets_reduce: bad arguments");
    hipStream_t st = emp_stream(stream);
    if (n == 0) return emp_zero_count(n_out, st, "triplets_reduce: memset");
    EMP_REQUIRE(trip && work && out, "triplets_reduce: null pointer");
    TripWork L = trip_carve(work, n);
    EMP_REQUIRE(work_bytes >= L.total, "triplets_reduce: workspace too small");
    int grid = emp_grid(n, 256, 4096);
    EMP_LAUNCH(trip_keys_kernel, grid, 256, st, trip, n, L.keys_in, L.vals_in);
    int rc = emp_sort_u64_i32(L.keys_in, L.keys_out, L.vals_in, L.vals_out, n, 0, 64, L.cub, L.cub_bytes, stream);
    if (rc != EMP_OK) return rc;
    return emp_compact(
        L.head, n, L.pos, L.scantmp, n_out, stream, "triplets_reduce: count copy",
        [&]() -> int {
            EMP_LAUNCH(emp_heads_kernel<0>, grid, 256, st, L.keys_out, n, L.head);
            return EMP_OK;
        },
        [&]() -> int {
            EMP_LAUNCH(trip_emit_kernel, grid, 256, st, L.keys_out, L.vals_out, n, L.head, L.pos, out);
            return EMP_OK;
        });
}
