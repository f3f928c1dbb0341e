// Sparse overlap table of two label arrays: every distinct pair (g, p) != (0, 0) of gt[i], pred[i] with its voxel
// count, sorted by (g, p).  replaces the joint histogram behind the reference's scores -- rle_matcher's IoU matrix
// (inference/matcher.py:136-232) as the Evaluator calls it (evaluation/evaluator.py:88-89) for the metrics of
// evaluation/panoptic_metrics.py:3-54 that scripts/evaluate3d.py:204-218 prints.
//
// Same shape as the run extractor of emp_runs.hip: count the spans of constant pair per row (ballots + a carried last
// pair), scan the row counts, extract (key = g << 32 | p, length) to row_offset + i, sort by key, sum equal keys.  The
// two passes over the voxels read sizeof(gt) + sizeof(pred) bytes per voxel each and that is the whole per-voxel
// traffic; everything after them is O(#spans).  No table is sized by a guess: the scan's total is the span count.
#include "emp_common.h"

// ------------------------------------------------------------------------------------------ spans of constant pair
// One wave per row; each lane owns VEC consecutive voxels of both arrays.  VEC = 4: the lane grid of a row starts at
// -shift, shift = (element index of the row's first voxel) mod 4, so that every full group of 4 is one aligned load
// (16 bytes of uint32, 4 bytes of uint8) for ANY W; the groups cut by the row's two ends are read voxel by voxel.
// VEC = 1 serves arrays whose base addresses sit at different element offsets mod 4.  Voxels outside the row read
// as the pair (0, 0), which neither starts nor ends a span, so no other bounds test is needed.
template <typename T, int VEC>
__device__ __forceinline__ void ov_fetch(const T *__restrict__ src, int64_t x, int64_t W, uint32_t (&v)[VEC])
{
    if constexpr (VEC == 4) {
        if (x >= 0 && x + 4 <= W) {
            if constexpr (sizeof(T) == 4) {
                const uint4 q = *reinterpret_cast<const uint4 *>(src + x);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                const uint32_t q = *reinterpret_cast<const uint32_t *>(src + x);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (q >> (8 * j)) & 0xffu;
            }
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = (x + j >= 0 && x + j < W) ? (uint32_t)src[x + j] : 0u;
}

template <typename TG, typename TP, int VEC, bool EXTRACT>
__global__ __launch_bounds__(256) void ov_spans_kernel(const TG *__restrict__ gt, const TP *__restrict__ pred,
                                                       int64_t n_rows, int64_t W, int align0,
                                                       int32_t *__restrict__ row_counts,
                                                       const int32_t *__restrict__ row_offsets,
                                                       uint64_t *__restrict__ s_key, int32_t *__restrict__ s_start,
                                                       int32_t *__restrict__ s_end)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;            // lanes before this one
    for (int64_t row = wave; row < n_rows; row += n_waves) {
        const TG *sg = gt + row * W;
        const TP *sp = pred + row * W;
        const int shift = VEC == 4 ? (int)((align0 + row * W) & 3) : 0;
        int n_s = 0, n_e = 0;  // wave-uniform running counts of starts / ends in this row
        const int32_t obase = EXTRACT ? row_offsets[row] : 0;
        // as in row_runs_kernel: the next chunk is requested before the current one is scanned, and the neighbours a
        // lane cannot get from the lane beside it come from the chunks in registers
        uint32_t cg[VEC], cp[VEC], ng[VEC], np[VEC];
        ov_fetch<TG, VEC>(sg, (int64_t)lane * VEC - shift, W, cg);
        ov_fetch<TP, VEC>(sp, (int64_t)lane * VEC - shift, W, cp);
        uint32_t carry_g = 0u, carry_p = 0u;                            // voxel left of the chunk ((0, 0) at the row start)
        for (int64_t x0 = -shift; x0 < W; x0 += 64 * VEC) {
            const int64_t x = x0 + (int64_t)lane * VEC;
            if (x0 + 64 * VEC < W) {
                ov_fetch<TG, VEC>(sg, x + 64 * VEC, W, ng);
                ov_fetch<TP, VEC>(sp, x + 64 * VEC, W, np);
            } else {
#pragma unroll
                for (int j = 0; j < VEC; ++j) ng[j] = np[j] = 0u;
            }
            uint32_t g[VEC + 2], p[VEC + 2];  // [0] = left neighbour, [VEC + 1] = right neighbour
#pragma unroll
            for (int j = 0; j < VEC; ++j) { g[j + 1] = cg[j]; p[j + 1] = cp[j]; }
            uint32_t lg = __shfl_up(cg[VEC - 1], 1), lp = __shfl_up(cp[VEC - 1], 1);
            uint32_t rg = __shfl_down(cg[0], 1), rp = __shfl_down(cp[0], 1);
            const uint32_t fg = __shfl(ng[0], 0), fp = __shfl(np[0], 0);
            if (lane == 0) { lg = carry_g; lp = carry_p; }
            if (lane == 63) { rg = fg; rp = fp; }                       // (0, 0) past the row's end
            g[0] = lg; p[0] = lp;
            g[VEC + 1] = rg; p[VEC + 1] = rp;
            bool st[VEC], en[VEC];
            unsigned long long bs[VEC], be[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const bool nz = (g[j + 1] | p[j + 1]) != 0u;
                st[j] = nz && (g[j + 1] != g[j] || p[j + 1] != p[j]);
                en[j] = nz && (g[j + 1] != g[j + 2] || p[j + 1] != p[j + 2]);
                bs[j] = __ballot(st[j]);
                be[j] = __ballot(en[j]);
            }
            int tot_s = 0, tot_e = 0, ps = 0, pe = 0;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                tot_s += __popcll(bs[j]);
                tot_e += __popcll(be[j]);
                if (EXTRACT) {
                    ps += __popcll(bs[j] & below);
                    pe += __popcll(be[j] & below);
                }
            }
            if (EXTRACT) {
                int is = obase + n_s + ps, ie = obase + n_e + pe;
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    if (st[j]) {
                        s_key[is] = ((uint64_t)g[j + 1] << 32) | (uint64_t)p[j + 1];   // both unsigned: no sign extension
                        s_start[is] = (int32_t)(x + j);
                        ++is;
                    }
                    if (en[j]) { s_end[ie] = (int32_t)(x + j + 1); ++ie; }             // exclusive end, made a length below
                }
            }
            n_s += tot_s;
            n_e += tot_e;
            carry_g = __shfl(cg[VEC - 1], 63);
            carry_p = __shfl(cp[VEC - 1], 63);
#pragma unroll
            for (int j = 0; j < VEC; ++j) { cg[j] = ng[j]; cp[j] = np[j]; }
        }
        if (!EXTRACT && lane == 0) row_counts[row] = n_s;
    }
}

__global__ void ov_fix_len_kernel(const int32_t *__restrict__ s_start, int32_t *__restrict__ s_len, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        s_len[i] -= s_start[i];
}

static int ov_align0(const void *ptr, int elem) { return (int)((reinterpret_cast<uintptr_t>(ptr) / (uintptr_t)elem) & 3); }

template <typename TG, typename TP, bool EXTRACT>
static int ov_launch(const void *gt, const void *pred, int64_t R, int64_t W, int32_t *row_counts,
                     const int32_t *row_offsets, uint64_t *s_key, int32_t *s_start, int32_t *s_end, hipStream_t st)
{
    const TG *g = reinterpret_cast<const TG *>(gt);
    const TP *p = reinterpret_cast<const TP *>(pred);
    const int grid = emp_grid(R * 64, 256, 16384);
    const int ag = ov_align0(gt, sizeof(TG)), ap = ov_align0(pred, sizeof(TP));
    // wide loads need the row's groups of 4 to be aligned in BOTH arrays at once: equal element offsets mod 4, and
    // (uint8) a base that is itself a whole number of elements -- always true -- so the offsets alone decide
    if (ag == ap)
        EMP_LAUNCH((ov_spans_kernel<TG, TP, 4, EXTRACT>), grid, 256, st, g, p, R, W, ag, row_counts, row_offsets, s_key,
                   s_start, s_end);
    else
        EMP_LAUNCH((ov_spans_kernel<TG, TP, 1, EXTRACT>), grid, 256, st, g, p, R, W, 0, row_counts, row_offsets, s_key,
                   s_start, s_end);
    return EMP_OK;
}

template <bool EXTRACT>
static int ov_dispatch(const void *gt, int gt_bytes, const void *pred, int pred_bytes, int64_t R, int64_t W,
                       int32_t *row_counts, const int32_t *row_offsets, uint64_t *s_key, int32_t *s_start,
                       int32_t *s_end, hipStream_t st)
{
    if (gt_bytes == 4 && pred_bytes == 4)
        return ov_launch<uint32_t, uint32_t, EXTRACT>(gt, pred, R, W, row_counts, row_offsets, s_key, s_start, s_end, st);
    if (gt_bytes == 4 && pred_bytes == 1)
        return ov_launch<uint32_t, uint8_t, EXTRACT>(gt, pred, R, W, row_counts, row_offsets, s_key, s_start, s_end, st);
    if (gt_bytes == 1 && pred_bytes == 4)
        return ov_launch<uint8_t, uint32_t, EXTRACT>(gt, pred, R, W, row_counts, row_offsets, s_key, s_start, s_end, st);
    return ov_launch<uint8_t, uint8_t, EXTRACT>(gt, pred, R, W, row_counts, row_offsets, s_key, s_start, s_end, st);
}

// shared argument checks of the two entry points; the span total of a call is at most one per voxel, so R * W inside
// int32 keeps the scan's int32 total exact whatever the labels are
#define OV_REQUIRE_SHAPE(what)                                                                                       \
    do {                                                                                                             \
        EMP_REQUIRE(gt && pred, what ": null pointer");                                                              \
        EMP_REQUIRE((gt_bytes == 1 || gt_bytes == 4) && (pred_bytes == 1 || pred_bytes == 4),                        \
                    what ": labels must be uint8 (1) or uint32 (4), got %d and %d bytes", gt_bytes, pred_bytes);     \
        EMP_REQUIRE(R >= 0 && W > 0, what ": bad shape (R = %lld, W = %lld)", (long long)R, (long long)W);           \
        EMP_REQUIRE(R == 0 || W <= 0x7fffffffLL / R,                                                                 \
                    what ": %lld x %lld voxels could hold more than 2^31 - 1 spans; split the rows into blocks",     \
                    (long long)R, (long long)W);                                                                     \
        EMP_REQUIRE((reinterpret_cast<uintptr_t>(gt) % (uintptr_t)gt_bytes) == 0 &&                                  \
                    (reinterpret_cast<uintptr_t>(pred) % (uintptr_t)pred_bytes) == 0, what ": misaligned labels");   \
    } while (0)

// ------------------------------------------------------------------------------------------ count + scan
extern "C" int64_t emp_label_overlaps_count_work_bytes(int64_t R) { return emp_count_carve(nullptr, R).total; }

extern "C" int emp_label_overlaps_count(const void *gt, int gt_bytes, const void *pred, int pred_bytes, int64_t R,
                                        int64_t W, void *work, int64_t work_bytes, int32_t *row_offsets, void *stream)
{
    OV_REQUIRE_SHAPE("label_overlaps_count");
    EMP_REQUIRE(work && row_offsets, "label_overlaps_count: null pointer");
    EmpCountWork L = emp_count_carve(work, R);
    EMP_REQUIRE(work_bytes >= L.total, "label_overlaps_count: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.total);
    hipStream_t st = emp_stream(stream);
    if (R == 0) {
        EMP_LAUNCH(emp_zero_kernel<int32_t>, 1, 64, st, row_offsets, (int64_t)1);
        return EMP_OK;
    }
    int rc = ov_dispatch<false>(gt, gt_bytes, pred, pred_bytes, R, W, L.counts, nullptr, nullptr, nullptr, nullptr, st);
    if (rc != EMP_OK) return rc;
    return emp_exclusive_scan_i32(L.counts, R, row_offsets, L.scantmp, stream);
}

// ------------------------------------------------------------------------------------------ extract + sort + reduce
// Every thread sums OV_SEG consecutive sorted spans and adds a partial sum to the pair's count wherever the key changes
// and at the segment's end: a pair that fills a million spans costs 1/OV_SEG as many atomics, and no thread walks a
// whole pair alone.  Integer adds, so the order of the atomics does not show in the result.
#define OV_SEG 16
__global__ void ov_reduce_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ lens, int64_t n,
                                 const int32_t *__restrict__ head, const int32_t *__restrict__ pos,
                                 int64_t *__restrict__ out_pairs, int64_t *__restrict__ out_counts)
{
    const int64_t n_seg = (n + OV_SEG - 1) / OV_SEG;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_seg; s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i0 = s * OV_SEG, i1 = (i0 + OV_SEG < n) ? i0 + OV_SEG : n;
        int64_t o = (int64_t)pos[i0] - (head[i0] ? 0 : 1);   // pos counts the heads BEFORE i: a span inside a pair sits
                                                             // one past its own head
        unsigned long long acc = 0ull;
        for (int64_t i = i0; i < i1; ++i) {
            if (head[i]) {
                if (i != i0) {
                    atomicAdd(reinterpret_cast<unsigned long long *>(&out_counts[o]), acc);
                    acc = 0ull;
                    o = pos[i];
                }
                out_pairs[2 * o] = (int64_t)(keys[i] >> 32);
                out_pairs[2 * o + 1] = (int64_t)(keys[i] & 0xffffffffULL);
            }
            acc += (unsigned long long)lens[i];
        }
        atomicAdd(reinterpret_cast<unsigned long long *>(&out_counts[o]), acc);
    }
}

struct OvWork {
    uint64_t *keys_in, *keys_out;
    int32_t *start, *lens_in, *lens_out, *head, *pos, *scantmp;
    char *cub;
    int64_t cub_bytes, total;
};
static OvWork ov_carve(void *work, int64_t n)
{
    if (n < 1) n = 1;
    EmpCarver c(work);
    OvWork L;
    L.keys_in = c.take<uint64_t>(n);
    L.keys_out = c.take<uint64_t>(n);
    L.lens_in = c.take<int32_t>(n);
    L.lens_out = c.take<int32_t>(n);
    L.head = c.take<int32_t>(n);
    L.start = L.head;                       // the span starts are dead (lengths fixed) before the heads are written
    L.pos = c.take<int32_t>(n + 1);
    L.scantmp = c.take<int32_t>(emp_scan_tmp_elems(n));
    L.cub_bytes = emp_sort_work_bytes(n);
    L.cub = c.take<char>(L.cub_bytes);
    L.total = c.bytes();
    return L;
}
extern "C" int64_t emp_label_overlaps_work_bytes(int64_t n_spans) { return ov_carve(nullptr, n_spans).total; }

extern "C" int emp_label_overlaps(const void *gt, int gt_bytes, const void *pred, int pred_bytes, int64_t R, int64_t W,
                                  const int32_t *row_offsets, int64_t n_spans, void *work, int64_t work_bytes,
                                  int64_t *out_pairs, int64_t *out_counts, int32_t *n_out, void *stream)
{
    OV_REQUIRE_SHAPE("label_overlaps");
    EMP_REQUIRE(row_offsets && n_out, "label_overlaps: null pointer");
    EMP_REQUIRE(n_spans >= 0 && n_spans <= R * W, "label_overlaps: n_spans = %lld is not the span total of %lld voxels",
                (long long)n_spans, (long long)(R * W));
    hipStream_t st = emp_stream(stream);
    if (n_spans == 0) {
        EMP_LAUNCH(emp_zero_kernel<int32_t>, 1, 64, st, n_out, (int64_t)1);
        return EMP_OK;
    }
    EMP_REQUIRE(work && out_pairs && out_counts, "label_overlaps: null pointer");
    OvWork L = ov_carve(work, n_spans);
    EMP_REQUIRE(work_bytes >= L.total, "label_overlaps: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.total);
    const int grid = emp_grid(n_spans, 256, 4096);
    int rc = ov_dispatch<true>(gt, gt_bytes, pred, pred_bytes, R, W, nullptr, row_offsets, L.keys_in, L.start, L.lens_in,
                               st);
    if (rc != EMP_OK) return rc;
    EMP_LAUNCH(ov_fix_len_kernel, grid, 256, st, L.start, L.lens_in, n_spans);
    rc = emp_sort_u64_i32(L.keys_in, L.keys_out, L.lens_in, L.lens_out, n_spans, 0, 64, L.cub, L.cub_bytes, stream);
    if (rc != EMP_OK) return rc;
    EMP_LAUNCH(emp_zero_kernel<int64_t>, grid, 256, st, out_counts, n_spans);
    return emp_compact(
        L.head, n_spans, L.pos, L.scantmp, n_out, stream, "label_overlaps: count copy",
        [&]() -> int {
            EMP_LAUNCH(emp_heads_kernel<0>, grid, 256, st, L.keys_out, n_spans, L.head);
            return EMP_OK;
        },
        [&]() -> int {
            EMP_LAUNCH(ov_reduce_kernel, emp_grid(emp_cdiv(n_spans, OV_SEG), 256, 4096), 256, st, L.keys_out, L.lens_out,
                       n_spans, L.head, L.pos, out_pairs, out_counts);
            return EMP_OK;
        });
}
