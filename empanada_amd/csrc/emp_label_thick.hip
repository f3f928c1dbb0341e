// Local thickness of the labelled objects (include/emp_hip.h, E10): T2(p) = the largest capped squared distance d2(q)
// among the voxels q whose ball |p - q|^2 < d2(q) covers p -- the squared radius of the largest inscribed ball that
// COVERS a voxel, not of the one centred on it.  What users of the reference do on a CPU afterwards with ImageJ / BoneJ
// "Local Thickness" or an edt per object; the definition is the header's.
//
// d2 -> lists -> resolve, over the block extended by its halo stacks (Z = hb + D + ha slices, its end slices faces).
//   d2       emp_label_edt's three passes with every slice of the extended volume as output (emp_label_edt_extended).
//   lists    per tile of 8 x 8 x 64 voxels of the extended volume: th_count_kernel counts the voxels with d2 > 0 (the
//            candidates; nothing is pruned) and keeps the tile's largest d2; the counts are scanned; th_sort_kernel
//            sorts the tile's keys d2 << 12 | voxel-in-tile descending in LDS (bitonic, 4096 keys) and writes them at
//            the tile's offset.  The keys of a tile are distinct, so the list is the same from run to run.
//   resolve  one workgroup per tile that meets the core.  The tile's values live in LDS, starting as its own d2.  The
//            tile itself and then every tile within reach -- the weighted gap between the two boxes, squared, lies
//            below that tile's largest d2 -- hands over its list, 256 keys at a time, one ball per lane: the lane
//            walks the rows of its ball that meet the tile and raises every voxel in them with an LDS atomic max, so
//            a key costs the voxels its ball covers in this tile, not the tile.  Before each batch the block takes the
//            smallest value that a labelled voxel of the tile holds: the list is descending, so it is left at the
//            first batch whose keys are no larger than that, or than the squared gap to that tile.  No global
//            atomics: the result is a maximum, so no order shows in it.
// All arithmetic is integer.
#include "emp_common.h"

#define TH_THREADS 256
#define TH_TILE (EMP_TILE_Z * EMP_TILE_Y * EMP_TILE_X)      // 4096 voxels: the voxel-in-tile takes 12 bits of a key
#define TH_NONE 0x7fffffff                                   // above every d2: "no labelled voxel here"

struct ThGeom {
    int64_t Z, H, W, hb, D;             // extended volume; the core is its slices hb .. hb + D - 1
    int64_t ntz, nty, ntx, nt;
    int az2, ay2, ax2, cap;
    int rz, ry, rx;                     // reach in tiles: no ball of squared radius <= cap gets farther
};

struct ThWork {
    uint16_t *d2, *tmp;                 // the distance over the extended volume, and the edt's second buffer
    uint32_t *list;                     // the keys of all tiles, tile after tile
    int32_t *counts, *scantmp;          // EmpCountWork
    int32_t *offsets, *tmax;
    unsigned long long *totals;         // candidates, voxels of the core with d2 == cap, tiles with a list, longest list
    int64_t bytes;
};
static ThWork th_carve(void *work, int64_t n_ext, int64_t nt)
{
    if (n_ext < 1) n_ext = 1;
    if (nt < 1) nt = 1;
    EmpCarver c(work);
    ThWork L;
    L.d2 = c.take<uint16_t>(n_ext);
    L.tmp = c.take<uint16_t>(n_ext);
    L.list = c.take<uint32_t>(n_ext);
    char *cw = c.take<char>(emp_count_carve(nullptr, nt).total);
    const EmpCountWork C = emp_count_carve(cw, nt);
    L.counts = C.counts;
    L.scantmp = C.scantmp;
    L.offsets = c.take<int32_t>(nt + 1);
    L.tmax = c.take<int32_t>(nt);
    L.totals = c.take<unsigned long long>(4);
    L.bytes = c.bytes();
    return L;
}

__device__ __forceinline__ void th_tile_origin(const ThGeom &g, int64_t tile, int64_t &tz, int64_t &ty, int64_t &tx)
{
    tx = tile % g.ntx;
    const int64_t r = tile / g.ntx;
    ty = r % g.nty;
    tz = r / g.nty;
}

// ------------------------------------------------------------------------------------------ lists: count
__global__ __launch_bounds__(TH_THREADS) void th_count_kernel(const uint16_t *__restrict__ d2, ThGeom g,
                                                              int32_t *__restrict__ counts, int32_t *__restrict__ tmax,
                                                              unsigned long long *__restrict__ totals)
{
    __shared__ int s_n, s_mx, s_cap;
    const int t = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < g.nt; tile += gridDim.x) {
        int64_t tz, ty, tx;
        th_tile_origin(g, tile, tz, ty, tx);
        if (t == 0) s_n = s_mx = s_cap = 0;
        __syncthreads();
        int n = 0, mx = 0, cp = 0;
        const int64_t x = tx * EMP_TILE_X + (t & 63);
        if (x < g.W) {
            for (int k = 0; k < 16; ++k) {
                const int r = k * 4 + (t >> 6);
                const int64_t z = tz * EMP_TILE_Z + (r >> 3), y = ty * EMP_TILE_Y + (r & 7);
                if (z >= g.Z || y >= g.H) continue;
                const int v = d2[(z * g.H + y) * g.W + x];
                n += v != 0 ? 1 : 0;
                mx = v > mx ? v : mx;
                cp += (v == g.cap && z >= g.hb && z < g.hb + g.D) ? 1 : 0;
            }
        }
        if (n) {
            atomicAdd(&s_n, n);
            atomicMax(&s_mx, mx);
        }
        if (cp) atomicAdd(&s_cap, cp);
        __syncthreads();
        if (t == 0) {
            counts[tile] = s_n;
            tmax[tile] = s_mx;
            if (s_n) {
                atomicAdd(totals + 0, (unsigned long long)s_n);
                atomicAdd(totals + 2, 1ull);
                atomicMax(totals + 3, (unsigned long long)s_n);
            }
            if (s_cap) atomicAdd(totals + 1, (unsigned long long)s_cap);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ lists: sort and emit
__global__ __launch_bounds__(TH_THREADS) void th_sort_kernel(const uint16_t *__restrict__ d2, ThGeom g,
                                                             const int32_t *__restrict__ counts,
                                                             const int32_t *__restrict__ offsets, int64_t capacity,
                                                             uint32_t *__restrict__ list)
{
    __shared__ uint32_t s_key[TH_TILE];
    const int t = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < g.nt; tile += gridDim.x) {
        const int cnt = counts[tile];
        if (cnt <= 0) continue;                                   // block uniform
        int64_t tz, ty, tx;
        th_tile_origin(g, tile, tz, ty, tx);
        __syncthreads();                                          // the tile before is written out
        const int64_t x = tx * EMP_TILE_X + (t & 63);
        for (int k = 0; k < 16; ++k) {
            const int r = k * 4 + (t >> 6), idx = r * 64 + (t & 63);
            const int64_t z = tz * EMP_TILE_Z + (r >> 3), y = ty * EMP_TILE_Y + (r & 7);
            uint32_t v = 0u;
            if (x < g.W && z < g.Z && y < g.H) v = d2[(z * g.H + y) * g.W + x];
            s_key[idx] = v ? (v << 12) | (uint32_t)idx : 0u;
        }
        __syncthreads();
        for (int size = 2; size <= TH_TILE; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int i = t; i < TH_TILE / 2; i += TH_THREADS) {
                    const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), hi = lo + stride;
                    const bool desc = (lo & size) == 0;
                    const uint32_t a = s_key[lo], b = s_key[hi];
                    if (desc ? a < b : a > b) {
                        s_key[lo] = b;
                        s_key[hi] = a;
                    }
                }
                __syncthreads();
            }
        }
        const int64_t off = offsets[tile];
        for (int i = t; i < cnt && i < TH_TILE; i += TH_THREADS)
            if (off + i < capacity) list[off + i] = s_key[i];     // never past the totals of the count pass
    }
}

// ------------------------------------------------------------------------------------------ resolve
// smallest |b - a| over a in [a0, a1], b in [b0, b1]
__device__ __forceinline__ int th_gap(int a0, int a1, int b0, int b1)
{
    return b0 > a1 ? b0 - a1 : (a0 > b1 ? a0 - b1 : 0);
}

// the largest k >= 0 with w k^2 < rem, for rem > 0: a float estimate put right in integers
__device__ __forceinline__ int th_half(int rem, int w)
{
    int k = (int)sqrtf((float)(rem - 1) / (float)w);
    while (w * (k + 1) * (k + 1) < rem) ++k;
    while (k > 0 && w * k * k >= rem) --k;
    return k;
}

// The ball of squared radius q2 around (qz, qy, qx), in the tile's own coordinates, painted into the tile: every
// voxel of the tile with |p - q|^2 < q2 takes max(value, q2).  One lane paints one ball, row by row.
__device__ __forceinline__ void th_paint(uint32_t *s_best, const ThGeom &g, int qz, int qy, int qx, int q2)
{
    const int rz = th_half(q2, g.az2);
    const int z_lo = max(qz - rz, 0), z_hi = min(qz + rz, EMP_TILE_Z - 1);
    for (int z = z_lo; z <= z_hi; ++z) {
        const int rem_z = q2 - g.az2 * (z - qz) * (z - qz);             // > 0 by rz
        const int ry = th_half(rem_z, g.ay2);
        const int y_lo = max(qy - ry, 0), y_hi = min(qy + ry, EMP_TILE_Y - 1);
        for (int y = y_lo; y <= y_hi; ++y) {
            const int rem = rem_z - g.ay2 * (y - qy) * (y - qy);        // > 0 by ry
            const int rx = th_half(rem, g.ax2);
            const int x_lo = max(qx - rx, 0), x_hi = min(qx + rx, EMP_TILE_X - 1);
            uint32_t *row = s_best + (z * EMP_TILE_Y + y) * EMP_TILE_X;
            for (int x = x_lo; x <= x_hi; ++x) atomicMax(row + x, (uint32_t)q2);
        }
    }
}

__global__ __launch_bounds__(TH_THREADS) void th_resolve_kernel(const uint16_t *__restrict__ d2, ThGeom g,
                                                                const int32_t *__restrict__ counts,
                                                                const int32_t *__restrict__ offsets,
                                                                const int32_t *__restrict__ tmax, int64_t capacity,
                                                                const uint32_t *__restrict__ list, int64_t tz_first,
                                                                int64_t n_tiles, uint16_t *__restrict__ out)
{
    __shared__ uint32_t s_best[TH_TILE];
    __shared__ int s_low;
    const int t = threadIdx.x, lx = t & 63;
    const int64_t per_z = g.nty * g.ntx;
    for (int64_t ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
        const int64_t tile = tz_first * per_z + ti;
        int64_t tz, ty, tx;
        th_tile_origin(g, tile, tz, ty, tx);
        const int64_t z0 = tz * EMP_TILE_Z, y0 = ty * EMP_TILE_Y, x = tx * EMP_TILE_X + lx;
        __syncthreads();                                          // the tile before is written out
        uint32_t labelled = 0u;                                   // bit k: this thread's voxel k is a labelled one of the core
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {
            const int r = k * 4 + (t >> 6);
            const int64_t z = z0 + (r >> 3), y = y0 + (r & 7);
            uint32_t v = 0u;
            if (x < g.W && y < g.H && z < g.Z) v = d2[(z * g.H + y) * g.W + x];
            s_best[r * 64 + lx] = v;
            labelled |= (v != 0u && z >= g.hb && z < g.hb + g.D ? 1u : 0u) << k;
        }
        const int n_self = counts[tile];
        // the tile itself first -- it holds most of what covers its voxels -- then every tile whose largest ball can
        // reach it; all of this is block uniform
        const int n_steps = n_self > 0 ? (2 * g.rz + 1) * (2 * g.ry + 1) * (2 * g.rx + 1) : -1;
        for (int step = 0; step <= n_steps; ++step) {
            int dzt = 0, dyt = 0, dxt = 0;
            if (step > 0) {
                const int s = step - 1, nx = 2 * g.rx + 1, ny = 2 * g.ry + 1;
                dxt = s % nx - g.rx;
                dyt = (s / nx) % ny - g.ry;
                dzt = s / (nx * ny) - g.rz;
                if (dzt == 0 && dyt == 0 && dxt == 0) continue;
            }
            const int64_t nz = tz + dzt, ny_ = ty + dyt, nx_ = tx + dxt;
            if (nz < 0 || nz >= g.ntz || ny_ < 0 || ny_ >= g.nty || nx_ < 0 || nx_ >= g.ntx) continue;
            const int64_t other = (nz * g.nty + ny_) * g.ntx + nx_;
            const int tm = tmax[other];
            if (tm == 0) continue;
            int gap2;
            {
                const int gz = th_gap(0, 7, dzt * 8, dzt * 8 + 7), gy = th_gap(0, 7, dyt * 8, dyt * 8 + 7),
                          gx = th_gap(0, 63, dxt * 64, dxt * 64 + 63);
                gap2 = g.az2 * gz * gz + g.ay2 * gy * gy + g.ax2 * gx * gx;
            }
            if (gap2 >= tm) continue;                             // no ball of that tile gets here
            int cnt = counts[other];
            cnt = cnt > TH_TILE ? TH_TILE : cnt;
            const int64_t off = offsets[other];
            if (off < 0 || off + cnt > capacity) continue;        // never past the totals of the count pass
            // 256 keys at a time, one ball per lane.  Before each batch: the smallest value that a labelled voxel of
            // the tile holds; the list is descending, so a batch whose first key is no larger paints nothing new
            for (int i0 = 0; i0 < cnt; i0 += TH_THREADS) {
                __syncthreads();                                  // the batch before is painted
                if (t == 0) s_low = TH_NONE;
                __syncthreads();
                int low = TH_NONE;
                for (int k = 0; k < 16; ++k)
                    if ((labelled >> k) & 1u) low = min(low, (int)s_best[(k * 4 + (t >> 6)) * 64 + lx]);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) low = min(low, __shfl_xor(low, o));
                if (lx == 0) atomicMin(&s_low, low);
                __syncthreads();
                const int first = (int)(list[off + i0] >> 12);
                if (first <= s_low || first <= gap2) break;
                if (i0 + t < cnt) {
                    const uint32_t key = list[off + i0 + t];
                    const int q2 = (int)(key >> 12);
                    if (q2 > gap2)
                        th_paint(s_best, g, dzt * 8 + (int)((key >> 9) & 7u), dyt * 8 + (int)((key >> 6) & 7u),
                                 dxt * 64 + (int)(key & 63u), q2);
                }
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {
            const int r = k * 4 + (t >> 6);
            const int64_t z = z0 + (r >> 3), y = y0 + (r & 7);
            if (x < g.W && y < g.H && z >= g.hb && z < g.hb + g.D)
                out[((z - g.hb) * g.H + y) * g.W + x] = (uint16_t)s_best[r * 64 + lx];
        }
    }
}

// ------------------------------------------------------------------------------------------ entry points
static int th_isqrt(int v)
{
    int r = 0;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

static bool th_shape_ok(int64_t D, int64_t H, int64_t W, int64_t hb, int64_t ha)
{
    return D >= 0 && hb >= 0 && ha >= 0 && D <= 0x7fffffffLL && hb <= 0x7fffffffLL && ha <= 0x7fffffffLL &&
           emp_tiles_shape_ok(D + hb + ha, H, W);
}

#define TH_REQUIRE_SHAPE(what)                                                                                        \
    do {                                                                                                              \
        EMP_REQUIRE(D >= 0 && H > 0 && W > 0, what ": bad shape (D = %lld, H = %lld, W = %lld)", (long long)D,        \
                    (long long)H, (long long)W);                                                                      \
        EMP_REQUIRE(hb >= 0 && ha >= 0, what ": bad halo counts (%lld, %lld)", (long long)hb, (long long)ha);         \
        EMP_REQUIRE(th_shape_ok(D, H, W, hb, ha),                                                                     \
                    what ": (%lld + %lld + %lld) x %lld x %lld voxels exceed 2^31 - 1; cut the slab into z-blocks",   \
                    (long long)hb, (long long)D, (long long)ha, (long long)H, (long long)W);                          \
        EMP_REQUIRE(cap >= 1 && cap <= 65535, what ": cap = %d outside 1 .. 65535", cap);                             \
    } while (0)

static ThGeom th_geometry(int64_t D, int64_t H, int64_t W, int64_t hb, int64_t ha, int az, int ay, int ax, int cap)
{
    ThGeom g;
    g.Z = hb + D + ha;
    g.H = H;
    g.W = W;
    g.hb = hb;
    g.D = D;
    const EmpTiles T = emp_tiles(g.Z, H, W);
    g.ntz = T.nz;
    g.nty = T.ny;
    g.ntx = T.nx;
    g.nt = T.n;
    g.az2 = az * az;
    g.ay2 = ay * ay;
    g.ax2 = ax * ax;
    g.cap = cap;
    const int root = th_isqrt(cap - 1);                           // |o|^2 < d2 <= cap: no offset is longer
    g.rz = (root / az + EMP_TILE_Z - 1) / EMP_TILE_Z;
    g.ry = (root / ay + EMP_TILE_Y - 1) / EMP_TILE_Y;
    g.rx = (root / ax + EMP_TILE_X - 1) / EMP_TILE_X;
    return g;
}

extern "C" int64_t emp_label_thick_work_bytes(int64_t D, int64_t H, int64_t W, int64_t hb, int64_t ha)
{
    if (H < 1 || W < 1 || !th_shape_ok(D, H, W, hb, ha)) return -1;
    const int64_t Z = D + hb + ha;
    return th_carve(nullptr, Z * H * W, emp_tiles(Z, H, W).n).bytes;
}

#define TH_REQUIRE_WORK(what)                                                                                         \
    EMP_REQUIRE(work, what ": null pointer");                                                                         \
    const ThWork L = th_carve(work, (D + hb + ha) * H * W, emp_tiles(D + hb + ha, H, W).n);                           \
    EMP_REQUIRE(work_bytes >= L.bytes, what ": workspace too small (%lld < %lld)", (long long)work_bytes,             \
                (long long)L.bytes)

extern "C" int emp_label_thick_edt(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below,
                                   int64_t hb, const void *above, int64_t ha, int az, int ay, int ax, int cap,
                                   void *work, int64_t work_bytes, void *stream)
{
    EMP_REQUIRE_VOLUME("label_thick_edt");
    TH_REQUIRE_SHAPE("label_thick_edt");
    if (D == 0) return EMP_OK;
    TH_REQUIRE_WORK("label_thick_edt");
    return emp_label_edt_extended(lab, item, D, H, W, below, hb, above, ha, az, ay, ax, cap, L.d2, L.tmp, stream);
}

extern "C" int emp_label_thick_lists(int64_t D, int64_t H, int64_t W, int64_t hb, int64_t ha, int cap, void *work,
                                     int64_t work_bytes, int64_t *totals, void *stream)
{
    TH_REQUIRE_SHAPE("label_thick_lists");
    EMP_REQUIRE(totals, "label_thick_lists: null pointer");
    hipStream_t st = emp_stream(stream);
    if (D == 0) {
        EMP_LAUNCH(emp_zero_kernel<int64_t>, 1, 64, st, totals, (int64_t)4);
        return EMP_OK;
    }
    TH_REQUIRE_WORK("label_thick_lists");
    const ThGeom g = th_geometry(D, H, W, hb, ha, 1, 1, 1, cap);
    EMP_LAUNCH(emp_zero_kernel<unsigned long long>, 1, 64, st, L.totals, (int64_t)4);
    const int grid = (int)(g.nt < 16384 ? g.nt : 16384);
    EMP_LAUNCH(th_count_kernel, grid, TH_THREADS, st, (const uint16_t *)L.d2, g, L.counts, L.tmax, L.totals);
    int rc = emp_exclusive_scan_i32(L.counts, g.nt, L.offsets, L.scantmp, stream);
    if (rc != EMP_OK) return rc;
    EMP_LAUNCH(th_sort_kernel, grid, TH_THREADS, st, (const uint16_t *)L.d2, g, (const int32_t *)L.counts,
               (const int32_t *)L.offsets, g.Z * g.H * g.W, L.list);
    if (hipMemcpyAsync(totals, L.totals, 4 * sizeof(int64_t), hipMemcpyDeviceToDevice, st) != hipSuccess)
        EMP_FAIL(EMP_ELAUNCH, "label_thick_lists: totals copy");
    return EMP_OK;
}

extern "C" int emp_label_thick_resolve(int64_t D, int64_t H, int64_t W, int64_t hb, int64_t ha, int az, int ay, int ax,
                                       int cap, const void *work, int64_t work_bytes, uint16_t *out, void *stream)
{
    TH_REQUIRE_SHAPE("label_thick_resolve");
    EMP_REQUIRE(az >= 1 && az <= 16 && ay >= 1 && ay <= 16 && ax >= 1 && ax <= 16,
                "label_thick_resolve: sampling (%d, %d, %d) outside 1 .. 16", az, ay, ax);
    if (D == 0) return EMP_OK;
    EMP_REQUIRE(out, "label_thick_resolve: null pointer");
    EMP_REQUIRE(work, "label_thick_resolve: null pointer");
    const ThWork L = th_carve(const_cast<void *>(work), (D + hb + ha) * H * W, emp_tiles(D + hb + ha, H, W).n);
    EMP_REQUIRE(work_bytes >= L.bytes, "label_thick_resolve: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.bytes);
    const ThGeom g = th_geometry(D, H, W, hb, ha, az, ay, ax, cap);
    const int64_t tz_first = hb / EMP_TILE_Z, tz_last = (hb + D - 1) / EMP_TILE_Z;
    const int64_t n_tiles = (tz_last - tz_first + 1) * g.nty * g.ntx;
    EMP_LAUNCH(th_resolve_kernel, (int)(n_tiles < 65536 ? n_tiles : 65536), TH_THREADS, emp_stream(stream),
               (const uint16_t *)L.d2, g, (const int32_t *)L.counts, (const int32_t *)L.offsets, (const int32_t *)L.tmax,
               g.Z * g.H * g.W, (const uint32_t *)L.list, tz_first, n_tiles, out);
    return EMP_OK;
}
