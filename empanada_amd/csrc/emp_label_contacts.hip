// Contact sites between the objects of two label volumes, or of one (include/emp_hip.h, E9): one table row per ordered
// pair (a, b) of labels that lie within a ball of squared radius r2 of each other -- contact voxels, smallest squared
// distance, index sums and shared faces.  What users of the reference do on a CPU afterwards, pair by pair, with an edt or
// a dilation per object; the definition is the header's.
//
// List -> count -> scan -> emit -> (caller: sort) -> heads -> scan -> reduce.  Tiles are 8 x 8 x 64 voxels, 256 threads
// each.  lc_list_kernel flags the tiles in which A has a label and B's tile plus ring holds a label that can be a partner
// (two distinct labels in the same-volume case); only those are walked.  A walked tile stages B's tile and a ring of
// (hz, hy, hx) = isqrt(r2) / pitch voxels in LDS, together with the ball table as LDS offsets; positions outside the
// volume and its halo stacks read as 0, which is never a partner.  Every thread then walks the ball, in ascending d2, for
// its 16 voxels of A: lanes of a wave hold consecutive x, so every ball offset is one conflict-free LDS read.  A foreign
// label is a record at its FIRST offset: the last four labels of the voxel sit in registers, and a label that is not
// among them is searched for among the earlier offsets in LDS; eight offsets are fetched together, and a batch that
// shows nothing but 0, the voxel's own label and cached labels is left at once.  The count pass and the emit pass run the same walk; the
// emit pass takes its positions from the tile's scanned offset and one LDS counter, so the order of a tile's records
// depends on scheduling -- the table does not: every column is an integer sum or minimum over a run of equal keys.
#include "emp_common.h"

#define LC_TZ 8
#define LC_TY 8
#define LC_TX 64
#define LC_THREADS 256
#define LC_MAX_HALO 4
#define LC_MAX_BALL 729                 // (2 * 4 + 1)^3
#define LC_COLS 10
#define LC_CHUNK 8                      // sorted records per thread of the row reduce
#define LC_MAX_VOXELS 0x7fffffffLL      // the voxel number inside the block is an int32
#define LC_MAX_RECORDS 0x7fffffffLL

struct LcGeom {
    int64_t D, H, W, hb, ha;
    int hz, hy, hx;                     // ring, in voxels
    int sz, sy, sx;                     // extents of the staged block of B
    int nty, ntx;                       // tiles along y and x
    int64_t n_tiles;
    int same, face_mask, n_ball;        // face_mask: bit 2 axis + side for the axes with pitch^2 <= r2
    int az, ay, ax, r2;
};

struct LcWork {
    int32_t *flag, *pos, *list, *counts, *offsets, *scantmp;
    unsigned long long *total;
    int64_t bytes;
};
static LcWork lc_carve(void *work, int64_t nt)
{
    if (nt < 1) nt = 1;
    EmpCarver c(work);
    LcWork L;
    L.flag = c.take<int32_t>(nt);
    L.pos = c.take<int32_t>(nt + 1);
    L.list = c.take<int32_t>(nt);
    L.counts = c.take<int32_t>(nt);
    L.offsets = c.take<int32_t>(nt + 1);
    L.scantmp = c.take<int32_t>(emp_scan_tmp_elems(nt));
    L.total = c.take<unsigned long long>(1);
    L.bytes = c.bytes();
    return L;
}

struct LcOut {
    uint64_t *keys;                     // a << 32 | b
    int32_t *vox;                       // voxel number inside the block
    int32_t *d2f;                       // d2 << 6 | face bits
    int64_t n_records;
};

// B at (z, y, x): the slab, its halo stacks, or 0 outside of all of them
template <typename TB>
__device__ __forceinline__ uint32_t lc_read_b(const TB *__restrict__ B, const TB *__restrict__ below,
                                              const TB *__restrict__ above, const LcGeom &g, int64_t z, int64_t y, int64_t x)
{
    if (y < 0 || y >= g.H || x < 0 || x >= g.W) return 0u;
    if (z >= 0 && z < g.D) return (uint32_t)B[(z * g.H + y) * g.W + x];
    if (z < 0 && z >= -g.hb && below != nullptr) return (uint32_t)below[((g.hb + z) * g.H + y) * g.W + x];
    if (z >= g.D && z < g.D + g.ha && above != nullptr) return (uint32_t)above[((z - g.D) * g.H + y) * g.W + x];
    return 0u;
}

__device__ __forceinline__ void lc_tile_origin(const LcGeom &g, int64_t tile, int64_t &z0, int64_t &y0, int64_t &x0)
{
    const int64_t tx = tile % g.ntx, r = tile / g.ntx, ty = r % g.nty, tz = r / g.nty;
    z0 = tz * LC_TZ;
    y0 = ty * LC_TY;
    x0 = tx * LC_TX;
}

// ------------------------------------------------------------------------------------------ which tiles have work
template <typename TA, typename TB>
__global__ __launch_bounds__(LC_THREADS) void lc_list_kernel(const TA *__restrict__ A, const TB *__restrict__ B,
                                                             const TB *__restrict__ below, const TB *__restrict__ above,
                                                             LcGeom g, int32_t *__restrict__ flag,
                                                             unsigned long long *__restrict__ total)
{
    __shared__ uint32_t s_mn, s_mx;
    const int t = threadIdx.x;
    if (blockIdx.x == 0 && t == 0) *total = 0ull;
    for (int64_t tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        int64_t z0, y0, x0;
        lc_tile_origin(g, tile, z0, y0, x0);
        int any = 0;
        const int64_t x = x0 + (t & 63);
        if (x < g.W) {
            for (int k = 0; k < 16; ++k) {
                const int r = k * 4 + (t >> 6);
                const int64_t z = z0 + (r >> 3), y = y0 + (r & 7);
                if (z < g.D && y < g.H && A[(z * g.H + y) * g.W + x] != 0) any = 1;
            }
        }
        if (t == 0) {
            s_mn = 0xffffffffu;
            s_mx = 0u;
        }
        any = __syncthreads_or(any);
        if (any) {
            uint32_t mn = 0xffffffffu, mx = 0u;
            const int cells = g.sz * g.sy * g.sx;
            for (int i = t; i < cells; i += LC_THREADS) {
                const int cx = i % g.sx, q = i / g.sx, cy = q % g.sy, cz = q / g.sy;
                const uint32_t l = lc_read_b<TB>(B, below, above, g, z0 + cz - g.hz, y0 + cy - g.hy, x0 + cx - g.hx);
                if (l != 0u) {
                    mn = l < mn ? l : mn;
                    mx = l > mx ? l : mx;
                }
            }
            if (mx != 0u) {
                atomicMin(&s_mn, mn);
                atomicMax(&s_mx, mx);
            }
        }
        __syncthreads();
        if (t == 0) flag[tile] = any && (g.same ? s_mn < s_mx : s_mx != 0u) ? 1 : 0;
        __syncthreads();
    }
}

__global__ void lc_compact_kernel(const int32_t *__restrict__ flag, const int32_t *__restrict__ pos, int64_t n,
                                  int32_t *__restrict__ list, int32_t *__restrict__ counts)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        counts[i] = 0;
        if (flag[i]) list[pos[i]] = (int32_t)i;
    }
}

// ------------------------------------------------------------------------------------------ the walk
// The records of one voxel of A (label a, LDS cell c): one per foreign label of the ball, at the label's first offset.
template <bool EMIT>
__device__ __forceinline__ int lc_walk(const uint32_t *__restrict__ s, const int2 *__restrict__ s_ball, int c, uint32_t a,
                                       const LcGeom &g, int stz, int sty, const LcOut &o, int64_t base, int *s_cnt,
                                       int32_t vox)
{
    uint32_t c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u;        // the last labels met at this voxel; 0 is never a partner
    int n = 0;
    const int n8 = (g.n_ball + 7) & ~7;                 // the table is padded to eight with offsets that are not walked
    for (int i0 = 0; i0 < n8; i0 += 8) {
        // eight offsets at a time, their LDS reads in flight together: inside an object, and where the cached labels
        // are all there is, nothing of the batch needs a decision.  The cache only grows, so the test is safe.
        bool any = false;
        {
            int2 e8[8];
            uint32_t l8[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) e8[k] = s_ball[i0 + k];
#pragma unroll
            for (int k = 0; k < 8; ++k) l8[k] = s[c + e8[k].x];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t v = e8[k].y < 0 ? 0u : l8[k];
                any = any || (v != 0u && !(g.same && v == a) && v != c0 && v != c1 && v != c2 && v != c3);
            }
        }
        if (!any) continue;
        for (int i = i0; i < i0 + 8; ++i) {
            const int2 e = s_ball[i];
            if (e.y < 0) continue;                          // an offset outside the ring: not walked
            const uint32_t l = s[c + e.x];
            if (l == 0u || (g.same && l == a)) continue;
            if (l == c0 || l == c1 || l == c2 || l == c3) continue;
            bool seen = false;
            for (int j = 0; j < i; ++j) {
                const int2 f = s_ball[j];
                if (f.y >= 0 && s[c + f.x] == l) {
                    seen = true;
                    break;
                }
            }
            c3 = c2;
            c2 = c1;
            c1 = c0;
            c0 = l;
            if (seen) continue;
            if (EMIT) {
                int f = 0;
                if (g.face_mask & 1) f |= (s[c - stz] == l) ? 1 : 0;
                if (g.face_mask & 2) f |= (s[c + stz] == l) ? 2 : 0;
                if (g.face_mask & 4) f |= (s[c - sty] == l) ? 4 : 0;
                if (g.face_mask & 8) f |= (s[c + sty] == l) ? 8 : 0;
                if (g.face_mask & 16) f |= (s[c - 1] == l) ? 16 : 0;
                if (g.face_mask & 32) f |= (s[c + 1] == l) ? 32 : 0;
                const int64_t q = base + atomicAdd(s_cnt, 1);
                if (q < o.n_records) {                      // never past the totals of the count pass
                    o.keys[q] = ((uint64_t)a << 32) | (uint64_t)l;
                    o.vox[q] = vox;
                    o.d2f[q] = (e.y << 6) | f;
                }
            }
            ++n;
        }
    }
    return n;
}

template <typename TA, typename TB, bool EMIT>
__global__ __launch_bounds__(LC_THREADS) void lc_walk_kernel(const TA *__restrict__ A, const TB *__restrict__ B,
                                                             const TB *__restrict__ below, const TB *__restrict__ above,
                                                             LcGeom g, const int32_t *__restrict__ ball,
                                                             const int32_t *__restrict__ list,
                                                             const int32_t *__restrict__ n_listed_dev,
                                                             int32_t *__restrict__ counts,
                                                             const int32_t *__restrict__ offsets,
                                                             unsigned long long *__restrict__ total, LcOut o)
{
    // all of the LDS is dynamic, so that its base is aligned: B's block, the ball as (LDS offset, d2), the tile's counter
    extern __shared__ __attribute__((aligned(16))) uint32_t lc_lds[];
    const int cells = g.sz * g.sy * g.sx;
    uint32_t *s = lc_lds;
    int2 *s_ball = reinterpret_cast<int2 *>(lc_lds + ((cells + 3) & ~3));
    const int n8 = (g.n_ball + 7) & ~7;
    int *s_cnt_p = reinterpret_cast<int *>(s_ball + n8);
    const int t = threadIdx.x;
    const int sty = g.sx, stz = g.sy * g.sx;
    for (int i = t; i < n8; i += LC_THREADS) {
        const bool in = i < g.n_ball;
        const int dz = in ? ball[4 * i] : 0, dy = in ? ball[4 * i + 1] : 0, dx = in ? ball[4 * i + 2] : 0,
                  d2 = in ? ball[4 * i + 3] : -1;
        const bool ok = dz >= -g.hz && dz <= g.hz && dy >= -g.hy && dy <= g.hy && dx >= -g.hx && dx <= g.hx &&
                        d2 >= 0 && d2 <= g.r2;
        s_ball[i] = ok ? make_int2(dz * stz + dy * sty + dx, d2) : make_int2(0, -1);
    }
    int64_t n_listed = *n_listed_dev;
    if (n_listed > g.n_tiles) n_listed = g.n_tiles;
    for (int64_t li = blockIdx.x; li < n_listed; li += gridDim.x) {
        int64_t tile = list[li];
        if (tile < 0 || tile >= g.n_tiles) tile = 0;
        if (EMIT && offsets[li + 1] == offsets[li]) continue;      // block uniform: a listed tile without a record
        int64_t z0, y0, x0;
        lc_tile_origin(g, tile, z0, y0, x0);
        __syncthreads();                                           // the walk before is over: the block may be restaged
        if (t == 0) *s_cnt_p = 0;
        for (int i = t; i < cells; i += LC_THREADS) {
            const int cx = i % g.sx, q = i / g.sx, cy = q % g.sy, cz = q / g.sy;
            s[i] = lc_read_b<TB>(B, below, above, g, z0 + cz - g.hz, y0 + cy - g.hy, x0 + cx - g.hx);
        }
        __syncthreads();
        const int lx = t & 63;
        const int64_t x = x0 + lx;
        int n = 0;
        if (x < g.W) {
            for (int k = 0; k < 16; ++k) {
                const int r = k * 4 + (t >> 6), lz = r >> 3, ly = r & 7;
                const int64_t z = z0 + lz, y = y0 + ly;
                if (z >= g.D || y >= g.H) continue;
                const int64_t v = (z * g.H + y) * g.W + x;
                const uint32_t a = (uint32_t)A[v];
                if (a == 0u) continue;
                n += lc_walk<EMIT>(s, s_ball, (lz + g.hz) * stz + (ly + g.hy) * sty + lx + g.hx, a, g, stz, sty, o,
                                   EMIT ? (int64_t)offsets[li] : 0, s_cnt_p, (int32_t)v);
            }
        }
        if (!EMIT) {
            if (n) atomicAdd(s_cnt_p, n);
            __syncthreads();
            if (t == 0) {
                const int tile_total = *s_cnt_p;
                counts[li] = tile_total;
                if (tile_total) atomicAdd(total, (unsigned long long)tile_total);
            }
        }
    }
}

__global__ void lc_totals_kernel(const int32_t *__restrict__ n_listed, const unsigned long long *__restrict__ total,
                                 int64_t *__restrict__ totals)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        totals[0] = n_listed ? (int64_t)*n_listed : 0;
        totals[1] = total ? (int64_t)*total : 0;
    }
}

// ------------------------------------------------------------------------------------------ entry points: count, emit
static int lc_isqrt(int v)
{
    int r = 0;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

static int lc_geometry(const char *what, const void *a, int item_a, const void *b, int item_b, int64_t D, int64_t H,
                       int64_t W, const void *below, int64_t hb, const void *above, int64_t ha, int same, int az, int ay,
                       int ax, int r2, const int32_t *ball, int n_ball, LcGeom &g)
{
    EMP_REQUIRE(a && b, "%s: null pointer", what);
    EMP_REQUIRE((item_a == 1 || item_a == 4) && (item_b == 1 || item_b == 4),
                "%s: labels must be uint8 (1) or uint32 (4), got %d and %d bytes", what, item_a, item_b);
    EMP_REQUIRE(D >= 0 && H > 0 && W > 0, "%s: bad shape (D = %lld, H = %lld, W = %lld)", what, (long long)D,
                (long long)H, (long long)W);
    EMP_REQUIRE(H <= LC_MAX_VOXELS / W && (D == 0 || H * W <= LC_MAX_VOXELS / D),
                "%s: %lld x %lld x %lld voxels exceed 2^31 - 1 per call; cut the slab into z-blocks", what, (long long)D,
                (long long)H, (long long)W);
    EMP_REQUIRE(same == 0 || same == 1, "%s: same must be 0 or 1, got %d", what, same);
    EMP_REQUIRE(!same || (a == b && item_a == item_b), "%s: same = 1 with two different volumes", what);
    EMP_REQUIRE(az >= 1 && az <= 16 && ay >= 1 && ay <= 16 && ax >= 1 && ax <= 16,
                "%s: the sampling must lie in 1 .. 16, got (%d, %d, %d)", what, az, ay, ax);
    const int amin = az < ay ? (az < ax ? az : ax) : (ay < ax ? ay : ax);
    EMP_REQUIRE(r2 >= amin * amin, "%s: r2 = %d is below the smallest squared pitch: the ball is a point", what, r2);
    EMP_REQUIRE(r2 < (1 << 24), "%s: r2 = %d is out of range", what, r2);
    const int root = lc_isqrt(r2);
    EMP_REQUIRE(root / amin <= LC_MAX_HALO, "%s: r2 = %d at sampling (%d, %d, %d) needs a ring of %d voxels, above %d",
                what, r2, az, ay, ax, root / amin, LC_MAX_HALO);
    EMP_REQUIRE(hb >= 0 && ha >= 0 && hb <= root / az && ha <= root / az,
                "%s: halo stacks of %lld and %lld slices, the ball reaches %d", what, (long long)hb, (long long)ha,
                root / az);
    EMP_REQUIRE((hb == 0 || below) && (ha == 0 || above), "%s: a halo stack is null", what);
    EMP_REQUIRE(reinterpret_cast<uintptr_t>(a) % (uintptr_t)item_a == 0 &&
                    reinterpret_cast<uintptr_t>(b) % (uintptr_t)item_b == 0 &&
                    (!below || reinterpret_cast<uintptr_t>(below) % (uintptr_t)item_b == 0) &&
                    (!above || reinterpret_cast<uintptr_t>(above) % (uintptr_t)item_b == 0),
                "%s: misaligned labels or halo stack", what);
    EMP_REQUIRE(ball && n_ball >= 1 && n_ball <= LC_MAX_BALL, "%s: the ball table holds %d offsets, 1 .. %d expected", what,
                n_ball, LC_MAX_BALL);
    g.D = D;
    g.H = H;
    g.W = W;
    g.hb = hb;
    g.ha = ha;
    g.hz = root / az;
    g.hy = root / ay;
    g.hx = root / ax;
    g.sz = LC_TZ + 2 * g.hz;
    g.sy = LC_TY + 2 * g.hy;
    g.sx = LC_TX + 2 * g.hx;
    const int64_t ntz = emp_cdiv(D, LC_TZ), nty = emp_cdiv(H, LC_TY), ntx = emp_cdiv(W, LC_TX);
    g.nty = (int)nty;
    g.ntx = (int)ntx;
    g.n_tiles = ntz * nty * ntx;
    g.same = same;
    g.face_mask = (g.hz >= 1 ? 3 : 0) | (g.hy >= 1 ? 12 : 0) | (g.hx >= 1 ? 48 : 0);
    g.n_ball = n_ball;
    g.az = az;
    g.ay = ay;
    g.ax = ax;
    g.r2 = r2;
    return EMP_OK;
}

static size_t lc_lds_bytes(const LcGeom &g)
{
    const int cells = g.sz * g.sy * g.sx;
    return (size_t)((cells + 3) & ~3) * sizeof(uint32_t) + (size_t)((g.n_ball + 7) & ~7) * sizeof(int2) + 16;
}

extern "C" int64_t emp_label_contacts_work_bytes(int64_t D, int64_t H, int64_t W)
{
    if (D < 0 || H <= 0 || W <= 0 || H > LC_MAX_VOXELS / W || (D > 0 && H * W > LC_MAX_VOXELS / D)) return -1;
    return lc_carve(nullptr, emp_cdiv(D, LC_TZ) * emp_cdiv(H, LC_TY) * emp_cdiv(W, LC_TX)).bytes;
}

template <typename TA, typename TB, bool EMIT>
static int lc_launch_walk(const void *a, const void *b, const void *below, const void *above, const LcGeom &g,
                          const int32_t *ball, const LcWork &L, int64_t blocks, const LcOut &o, hipStream_t st)
{
    const size_t lds = lc_lds_bytes(g);
    if (lds > 64 * 1024)
        hipFuncSetAttribute((const void *)lc_walk_kernel<TA, TB, EMIT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
    hipLaunchKernelGGL((lc_walk_kernel<TA, TB, EMIT>), dim3((unsigned)blocks), dim3(LC_THREADS), lds, st,
                       reinterpret_cast<const TA *>(a), reinterpret_cast<const TB *>(b),
                       reinterpret_cast<const TB *>(below), reinterpret_cast<const TB *>(above), g, ball, L.list,
                       L.pos + g.n_tiles, L.counts, L.offsets, L.total, o);
    EMP_CHECK_LAUNCH("lc_walk_kernel");
    return EMP_OK;
}

template <bool EMIT>
static int lc_dispatch_walk(int item_a, int item_b, const void *a, const void *b, const void *below, const void *above,
                            const LcGeom &g, const int32_t *ball, const LcWork &L, int64_t blocks, const LcOut &o,
                            hipStream_t st)
{
    if (item_a == 4)
        return item_b == 4 ? lc_launch_walk<uint32_t, uint32_t, EMIT>(a, b, below, above, g, ball, L, blocks, o, st)
                           : lc_launch_walk<uint32_t, uint8_t, EMIT>(a, b, below, above, g, ball, L, blocks, o, st);
    return item_b == 4 ? lc_launch_walk<uint8_t, uint32_t, EMIT>(a, b, below, above, g, ball, L, blocks, o, st)
                       : lc_launch_walk<uint8_t, uint8_t, EMIT>(a, b, below, above, g, ball, L, blocks, o, st);
}

template <typename TA, typename TB>
static int lc_launch_list(const void *a, const void *b, const void *below, const void *above, const LcGeom &g,
                          const LcWork &L, hipStream_t st)
{
    EMP_LAUNCH((lc_list_kernel<TA, TB>), emp_grid(g.n_tiles * LC_THREADS, LC_THREADS, 16384), LC_THREADS, st,
               reinterpret_cast<const TA *>(a), reinterpret_cast<const TB *>(b), reinterpret_cast<const TB *>(below),
               reinterpret_cast<const TB *>(above), g, L.flag, L.total);
    return EMP_OK;
}

extern "C" int emp_label_contacts_count(const void *a, int item_a, const void *b, int item_b, int64_t D, int64_t H,
                                        int64_t W, const void *below, int64_t hb, const void *above, int64_t ha, int same,
                                        int az, int ay, int ax, int r2, const int32_t *ball, int n_ball, void *work,
                                        int64_t work_bytes, int64_t *totals, void *stream)
{
    LcGeom g;
    int rc = lc_geometry("label_contacts_count", a, item_a, b, item_b, D, H, W, below, hb, above, ha, same, az, ay, ax,
                         r2, ball, n_ball, g);
    if (rc != EMP_OK) return rc;
    EMP_REQUIRE(totals, "label_contacts_count: null pointer");
    hipStream_t st = emp_stream(stream);
    if (D == 0) {
        EMP_LAUNCH(lc_totals_kernel, 1, 64, st, (const int32_t *)nullptr, (const unsigned long long *)nullptr, totals);
        return EMP_OK;
    }
    EMP_REQUIRE(work, "label_contacts_count: null pointer");
    LcWork L = lc_carve(work, g.n_tiles);
    EMP_REQUIRE(work_bytes >= L.bytes, "label_contacts_count: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.bytes);
    const int64_t nt = g.n_tiles;
    rc = emp_compact(
        L.flag, nt, L.pos, L.scantmp, L.offsets /* scratch: overwritten by the scan below */, stream,
        "label_contacts_count: count copy",
        [&]() -> int {
            if (item_a == 4)
                return item_b == 4 ? lc_launch_list<uint32_t, uint32_t>(a, b, below, above, g, L, st)
                                   : lc_launch_list<uint32_t, uint8_t>(a, b, below, above, g, L, st);
            return item_b == 4 ? lc_launch_list<uint8_t, uint32_t>(a, b, below, above, g, L, st)
                               : lc_launch_list<uint8_t, uint8_t>(a, b, below, above, g, L, st);
        },
        [&]() -> int {
            EMP_LAUNCH(lc_compact_kernel, emp_grid(nt, 256, 4096), 256, st, L.flag, L.pos, nt, L.list, L.counts);
            return EMP_OK;
        });
    if (rc != EMP_OK) return rc;
    const LcOut none = {};
    rc = lc_dispatch_walk<false>(item_a, item_b, a, b, below, above, g, ball, L, nt < 8192 ? nt : 8192, none, st);
    if (rc != EMP_OK) return rc;
    rc = emp_exclusive_scan_i32(L.counts, nt, L.offsets, L.scantmp, stream);
    if (rc != EMP_OK) return rc;
    EMP_LAUNCH(lc_totals_kernel, 1, 64, st, (const int32_t *)(L.pos + nt), (const unsigned long long *)L.total, totals);
    return EMP_OK;
}

extern "C" int emp_label_contacts_emit(const void *a, int item_a, const void *b, int item_b, int64_t D, int64_t H,
                                       int64_t W, const void *below, int64_t hb, const void *above, int64_t ha, int same,
                                       int az, int ay, int ax, int r2, const int32_t *ball, int n_ball, void *work,
                                       int64_t work_bytes, int64_t n_listed, int64_t n_records, uint64_t *keys,
                                       int32_t *vox, int32_t *d2f, void *stream)
{
    LcGeom g;
    int rc = lc_geometry("label_contacts_emit", a, item_a, b, item_b, D, H, W, below, hb, above, ha, same, az, ay, ax,
                         r2, ball, n_ball, g);
    if (rc != EMP_OK) return rc;
    EMP_REQUIRE(n_listed >= 0 && n_listed <= g.n_tiles, "label_contacts_emit: %lld listed tiles of %lld",
                (long long)n_listed, (long long)g.n_tiles);
    EMP_REQUIRE(n_records >= 0 && n_records <= LC_MAX_RECORDS,
                "label_contacts_emit: %lld records: a call must stay below 2^31; cut the slab into smaller z-blocks",
                (long long)n_records);
    if (n_records == 0 || n_listed == 0) return EMP_OK;
    EMP_REQUIRE(work && keys && vox && d2f, "label_contacts_emit: null pointer");
    LcWork L = lc_carve(work, g.n_tiles);
    EMP_REQUIRE(work_bytes >= L.bytes, "label_contacts_emit: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.bytes);
    LcOut o;
    o.keys = keys;
    o.vox = vox;
    o.d2f = d2f;
    o.n_records = n_records;
    return lc_dispatch_walk<true>(item_a, item_b, a, b, below, above, g, ball, L, n_listed < 8192 ? n_listed : 8192, o,
                                  emp_stream(stream));
}

// ------------------------------------------------------------------------------------------ rows of the sorted records
__global__ void lc_rows_init_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ head,
                                    const int32_t *__restrict__ pos, int64_t n, int64_t *__restrict__ table,
                                    int64_t n_rows)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (!head[i]) continue;
        const int64_t row = pos[i];
        if (row >= n_rows) continue;
        int64_t *o = table + row * LC_COLS;
        const uint64_t k = keys[i];
        o[0] = (int64_t)(k >> 32);
        o[1] = (int64_t)(k & 0xffffffffULL);
        o[2] = 0;
        o[3] = 0x7fffffffffffffffLL;
#pragma unroll
        for (int c = 4; c < LC_COLS; ++c) o[c] = 0;
    }
}

struct LcAcc {
    unsigned long long n, sz, sy, sx, fz, fy, fx;
    long long mn;
};

__device__ __forceinline__ void lc_flush(int64_t *__restrict__ table, int64_t row, int64_t n_rows, const LcAcc &c)
{
    if (row < 0 || row >= n_rows || c.n == 0ull) return;
    unsigned long long *o = reinterpret_cast<unsigned long long *>(table + row * LC_COLS);
    atomicAdd(o + 2, c.n);
    atomicMin(reinterpret_cast<long long *>(o + 3), c.mn);
    atomicAdd(o + 4, c.sz);
    atomicAdd(o + 5, c.sy);
    atomicAdd(o + 6, c.sx);
    if (c.fz) atomicAdd(o + 7, c.fz);
    if (c.fy) atomicAdd(o + 8, c.fy);
    if (c.fx) atomicAdd(o + 9, c.fx);
}

// Every thread adds up LC_CHUNK consecutive sorted records and hands a run of equal keys to its row with one set of
// atomics: integer sums and a minimum, so the row does not depend on the order.
__global__ void lc_reduce_kernel(const int32_t *__restrict__ head, const int32_t *__restrict__ pos,
                                 const int32_t *__restrict__ perm, const int32_t *__restrict__ vox,
                                 const int32_t *__restrict__ d2f, int64_t n, int64_t H, int64_t W, int64_t z_base,
                                 int64_t *__restrict__ table, int64_t n_rows)
{
    const int64_t chunks = (n + LC_CHUNK - 1) / LC_CHUNK, HW = H * W;
    for (int64_t ch = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ch < chunks; ch += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i0 = ch * LC_CHUNK, i1 = i0 + LC_CHUNK < n ? i0 + LC_CHUNK : n;
        LcAcc c = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0x7fffffffffffffffLL};
        int64_t row = (int64_t)pos[i0] + head[i0] - 1;
        for (int64_t i = i0; i < i1; ++i) {
            if (i > i0 && head[i]) {
                lc_flush(table, row, n_rows, c);
                c = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0x7fffffffffffffffLL};
                ++row;
            }
            const int64_t p = perm[i];
            if (p < 0 || p >= n) continue;
            const int64_t v = vox[p];
            const int32_t df = d2f[p];
            const int64_t z = v / HW, rem = v - z * HW, y = rem / W;
            const long long d2 = df >> 6;
            c.n += 1ull;
            c.mn = d2 < c.mn ? d2 : c.mn;
            c.sz += (unsigned long long)(z + z_base);
            c.sy += (unsigned long long)y;
            c.sx += (unsigned long long)(rem - y * W);
            c.fz += (unsigned long long)__popc(df & 3);
            c.fy += (unsigned long long)__popc(df & 12);
            c.fx += (unsigned long long)__popc(df & 48);
        }
        lc_flush(table, row, n_rows, c);
    }
}

struct LcRowsWork {
    int32_t *head, *pos, *scantmp;
    int64_t bytes;
};
static LcRowsWork lc_rows_carve(void *work, int64_t n)
{
    if (n < 1) n = 1;
    EmpCarver c(work);
    LcRowsWork L;
    L.head = c.take<int32_t>(n);
    L.pos = c.take<int32_t>(n + 1);
    L.scantmp = c.take<int32_t>(emp_scan_tmp_elems(n));
    L.bytes = c.bytes();
    return L;
}
extern "C" int64_t emp_label_contacts_rows_work_bytes(int64_t n)
{
    if (n < 0 || n > LC_MAX_RECORDS) return -1;
    return lc_rows_carve(nullptr, n).bytes;
}

extern "C" int emp_label_contacts_rows(const uint64_t *keys, int64_t n, void *work, int64_t work_bytes, int32_t *n_rows,
                                       void *stream)
{
    EMP_REQUIRE(n >= 0 && n <= LC_MAX_RECORDS, "label_contacts_rows: %lld records: must stay below 2^31", (long long)n);
    EMP_REQUIRE(n_rows, "label_contacts_rows: null pointer");
    hipStream_t st = emp_stream(stream);
    if (n == 0) return emp_zero_count(n_rows, st, "label_contacts_rows: memset failed");
    EMP_REQUIRE(keys && work, "label_contacts_rows: null pointer");
    LcRowsWork L = lc_rows_carve(work, n);
    EMP_REQUIRE(work_bytes >= L.bytes, "label_contacts_rows: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.bytes);
    EMP_LAUNCH(emp_heads_kernel<0>, emp_grid(n, 256, 4096), 256, st, keys, n, L.head);
    int rc = emp_exclusive_scan_i32(L.head, n, L.pos, L.scantmp, stream);
    if (rc != EMP_OK) return rc;
    if (hipMemcpyAsync(n_rows, L.pos + n, sizeof(int32_t), hipMemcpyDeviceToDevice, st) != hipSuccess)
        EMP_FAIL(EMP_ELAUNCH, "label_contacts_rows: count copy");
    return EMP_OK;
}

extern "C" int emp_label_contacts_reduce(const uint64_t *keys, const int32_t *perm, const int32_t *vox,
                                         const int32_t *d2f, int64_t n, int64_t H, int64_t W, int64_t z_base,
                                         const void *work, int64_t work_bytes, int64_t *table, int64_t n_rows,
                                         void *stream)
{
    EMP_REQUIRE(n >= 0 && n <= LC_MAX_RECORDS, "label_contacts_reduce: %lld records: must stay below 2^31", (long long)n);
    EMP_REQUIRE(n_rows >= 0 && n_rows <= n, "label_contacts_reduce: %lld rows of %lld records", (long long)n_rows,
                (long long)n);
    EMP_REQUIRE(H > 0 && W > 0 && H <= LC_MAX_VOXELS / W, "label_contacts_reduce: bad shape (H = %lld, W = %lld)",
                (long long)H, (long long)W);
    EMP_REQUIRE(z_base >= 0 && z_base < (1LL << 40), "label_contacts_reduce: z_base = %lld", (long long)z_base);
    if (n == 0 || n_rows == 0) return EMP_OK;
    EMP_REQUIRE(keys && perm && vox && d2f && work && table, "label_contacts_reduce: null pointer");
    LcRowsWork L = lc_rows_carve(const_cast<void *>(work), n);
    EMP_REQUIRE(work_bytes >= L.bytes, "label_contacts_reduce: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.bytes);
    hipStream_t st = emp_stream(stream);
    EMP_LAUNCH(lc_rows_init_kernel, emp_grid(n, 256, 4096), 256, st, keys, L.head, L.pos, n, table, n_rows);
    EMP_LAUNCH(lc_reduce_kernel, emp_grid(emp_cdiv(n, LC_CHUNK), 256, 4096), 256, st, L.head, L.pos, perm, vox, d2f, n, H,
               W, z_base, table, n_rows);
    return EMP_OK;
}
