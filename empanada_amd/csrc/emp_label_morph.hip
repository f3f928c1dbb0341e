// Label morphology (include/emp_hip.h, E5): the capped squared Euclidean distance of every labelled voxel to the nearest
// voxel of another label, the erosion that thresholds it, and the nearest label within a ball for the dilation.  What
// users of the reference do on a CPU afterwards with scipy.ndimage.binary_opening or an edt per object; the definition
// is the header's.
//
// Both transforms are separable: three passes, x then y then z, over the slab extended by its halo stacks.  The x and
// y passes run over every slice, halos included, because the z pass of a core voxel reads the in-slice result of the
// halo slices; the z pass runs over the core alone and writes the output.  All arithmetic is integer and no kernel
// uses an atomic or waits for another block, so no launch shape shows in any output.
//   distance, x   one wave per row, 4 voxels per lane on the row's aligned grid: a forward sweep finds the start of
//                 every voxel's run of equal labels (segmented max-scan over the wave, carried from chunk to chunk), a
//                 backward sweep its end; the nearer label change, if the row has one on that side, gives the value.
//                 O(W) per row whatever the cap.
//   distance, y z one thread per voxel, lanes along x, so every step k is a coalesced read of a row; a side stops at
//                 the first voxel of another label (it is itself a candidate at w k^2 and all beyond it are farther)
//                 and at w k^2 >= best.
//   nearest       the key (d^2, label), smaller d^2 first, then the larger label; one thread per voxel in all three
//                 passes, k runs while w k^2 <= min(best d^2, r2) so that ties are seen.  A labelled voxel is done at
//                 once.
#include "emp_common.h"

#define MO_FAR 256                   // steps: w k^2 >= 65536 > cap for every k >= 256, so farther counts as "none"

// The slab with its halo stacks as one volume of Z = hb + D + ha slices
template <typename T> struct MoVol {
    const T *below, *lab, *above;
    int64_t hb, D, ha, HW;
    __device__ __forceinline__ const T *slice(int64_t ze) const
    {
        if (ze < hb) return below + ze * HW;
        if (ze < hb + D) return lab + (ze - hb) * HW;
        return above + (ze - hb - D) * HW;
    }
};

// ------------------------------------------------------------------------------------------ distance: x pass
// f[row][x] = min(cap, w k^2), k = steps to the nearest voxel of the row with another label (none on a side whose run
// reaches the row's end), 0 on zero voxels.  The forward sweep leaves the steps to the left in f, clamped to MO_FAR, and
// the backward sweep reads them back: both sweeps use the same chunk grid, so a lane reads what it wrote itself.
template <typename T>
__global__ __launch_bounds__(256) void mo_edt_rows_kernel(MoVol<T> vol, int64_t n_rows, int64_t H, int64_t W, int w, int cap,
                                                          uint16_t *__restrict__ f)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t row = wave; row < n_rows; row += n_waves) {
        const int64_t ze = row / H;
        const T *src = vol.slice(ze) + (row - ze * H) * W;
        uint16_t *dst = f + row * W;
        const int shift = (int)((reinterpret_cast<uintptr_t>(src) / sizeof(T)) & 3);
        uint32_t v[4];
        // forward: start of the run of equal labels that holds the voxel
        uint32_t carry_lab = 0u;
        int carry_pos = -1;
        for (int64_t x0 = -shift; x0 < W; x0 += 256) {
            const int64_t x = x0 + (int64_t)lane * 4;
            const uint32_t ok = emp_load4<T>(src, x, W, v);
            uint32_t pv = __shfl_up(v[3], 1);
            if (lane == 0) pv = carry_lab;
            int s[4], run = -1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool start = ((ok >> j) & 1u) && (x + j == 0 || v[j] != (j ? v[j - 1] : pv));
                if (start) run = (int)(x + j);
                s[j] = run;
            }
            int t = lane == 0 ? max(run, carry_pos) : run;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(t, d);
                if (lane >= d) t = max(t, o);
            }
            int before = __shfl_up(t, 1);
            if (lane == 0) before = carry_pos;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!((ok >> j) & 1u)) continue;
                const int st = s[j] < 0 ? before : s[j];
                const int64_t k = st <= 0 ? (int64_t)MO_FAR : min((int64_t)MO_FAR, x + j - st + 1);
                dst[x + j] = (uint16_t)k;
            }
            carry_lab = __shfl(v[3], 63);
            carry_pos = __shfl(t, 63);
        }
        // backward: end of the run, and the value
        const int64_t last = -shift + ((W - 1 + shift) / 256) * 256;
        const int none = 0x7fffffff;
        carry_lab = 0u;
        carry_pos = none;
        for (int64_t x0 = last; x0 >= -shift; x0 -= 256) {
            const int64_t x = x0 + (int64_t)lane * 4;
            const uint32_t ok = emp_load4<T>(src, x, W, v);
            uint32_t nv = __shfl_down(v[0], 1);
            if (lane == 63) nv = carry_lab;
            int e[4], run = none;
#pragma unroll
            for (int j = 3; j >= 0; --j) {
                const bool end = ((ok >> j) & 1u) && (x + j == W - 1 || v[j] != (j < 3 ? v[j + 1] : nv));
                if (end) run = (int)(x + j);
                e[j] = run;
            }
            int t = lane == 63 ? min(run, carry_pos) : run;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_down(t, d);
                if (lane + d < 64) t = min(t, o);
            }
            int after = __shfl_down(t, 1);
            if (lane == 63) after = carry_pos;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!((ok >> j) & 1u)) continue;
                const int64_t en = e[j] == none ? after : e[j];
                const int64_t kr = en >= W - 1 ? (int64_t)MO_FAR : min((int64_t)MO_FAR, en - (x + j) + 1);
                const int k = (int)min((int64_t)dst[x + j], kr);
                int val = 0;
                if (v[j] != 0u) val = k >= MO_FAR ? cap : min(cap, w * k * k);
                dst[x + j] = (uint16_t)val;
            }
            carry_lab = __shfl(v[0], 0);
            carry_pos = __shfl(t, 0);
        }
    }
}

// ------------------------------------------------------------------------------------------ distance: y and z passes
// One side of a line: the steps k = 1, 2, ... while w k^2 < best
template <typename T, typename Lab, typename Dist>
__device__ __forceinline__ int mo_edt_side(int best, uint32_t l, int w, int64_t n_steps, Lab lab_at, Dist f_at)
{
    for (int64_t k = 1; k <= n_steps; ++k) {
        const int wk2 = w * (int)k * (int)k;
        if (wk2 >= best) break;
        if (lab_at(k) != l) return wk2;
        best = min(best, f_at(k) + wk2);
    }
    return best;
}

template <typename T>
__global__ __launch_bounds__(256) void mo_edt_y_kernel(MoVol<T> vol, uint32_t n, uint32_t H, uint32_t W, int w,
                                                       const uint16_t *__restrict__ f, uint16_t *__restrict__ g)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t row = i / W, x = i - row * W, ze = row / H, y = row - ze * H;
        const T *src = vol.slice(ze) + x;
        const uint32_t l = (uint32_t)src[(int64_t)y * W];
        int best = 0;
        if (l != 0u) {
            const uint16_t *fs = f + (int64_t)ze * H * W + x;
            best = fs[(int64_t)y * W];
            if (best > w) {
                best = mo_edt_side<T>(
                    best, l, w, y, [&](int64_t k) { return (uint32_t)src[((int64_t)y - k) * W]; },
                    [&](int64_t k) { return (int)fs[((int64_t)y - k) * W]; });
                best = mo_edt_side<T>(
                    best, l, w, (int64_t)H - 1 - y, [&](int64_t k) { return (uint32_t)src[((int64_t)y + k) * W]; },
                    [&](int64_t k) { return (int)fs[((int64_t)y + k) * W]; });
            }
        }
        g[i] = (uint16_t)best;
    }
}

// the z pass over the core slices: g is indexed by the extended volume, the output by the core.  ERODE: the label
// where the distance exceeds r2 = cap - 1, 0 elsewhere, in the labels' own type; otherwise the distance as uint16.
// ALL: the output is indexed by the extended volume too (emp_label_edt_extended), every slice of it a core slice.
template <typename T, bool ERODE, bool ALL = false>
__global__ __launch_bounds__(256) void mo_edt_z_kernel(MoVol<T> vol, uint32_t n, uint32_t HW, int w, int cap,
                                                       const uint16_t *__restrict__ g, void *__restrict__ out)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    const int64_t Z = vol.hb + vol.D + vol.ha;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t z = i / HW, p = i - z * HW;
        const int64_t ze = ALL ? (int64_t)z : (int64_t)z + vol.hb;
        const uint32_t l = ALL ? (uint32_t)vol.slice(ze)[p] : (uint32_t)vol.lab[i];
        int best = 0;
        if (l != 0u) {
            best = g[ze * HW + p];
            if (best > w) {
                best = mo_edt_side<T>(
                    best, l, w, ze, [&](int64_t k) { return (uint32_t)vol.slice(ze - k)[p]; },
                    [&](int64_t k) { return (int)g[(ze - k) * HW + p]; });
                best = mo_edt_side<T>(
                    best, l, w, Z - 1 - ze, [&](int64_t k) { return (uint32_t)vol.slice(ze + k)[p]; },
                    [&](int64_t k) { return (int)g[(ze + k) * HW + p]; });
            }
        }
        if constexpr (ERODE)
            reinterpret_cast<T *>(out)[i] = best >= cap ? (T)l : (T)0;
        else
            reinterpret_cast<uint16_t *>(out)[i] = (uint16_t)best;
    }
}

// ------------------------------------------------------------------------------------------ nearest label
// the key (d, l) improves on (bd, bl): smaller distance, or the same distance and the larger label
__device__ __forceinline__ void mo_take(int &bd, uint32_t &bl, int d, uint32_t l)
{
    if (d < bd || (d == bd && l > bl)) {
        bd = d;
        bl = l;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void mo_near_x_kernel(MoVol<T> vol, uint32_t n, uint32_t H, uint32_t W, int w, int r2,
                                                        uint16_t *__restrict__ kd, uint32_t *__restrict__ kl)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t row = i / W, x = i - row * W, ze = row / H, y = row - ze * H;
        const T *src = vol.slice(ze) + (int64_t)y * W;
        int bd = 0;
        uint32_t bl = (uint32_t)src[x];
        if (bl == 0u) {
            bd = r2 + 1;
            for (int64_t k = 1;; ++k) {
                const int wk2 = w * (int)k * (int)k;
                const bool left = (int64_t)x - k >= 0, right = (int64_t)x + k < (int64_t)W;
                if (wk2 > min(bd, r2) || !(left || right)) break;
                if (left) {
                    const uint32_t u = (uint32_t)src[(int64_t)x - k];
                    if (u != 0u) mo_take(bd, bl, wk2, u);
                }
                if (right) {
                    const uint32_t u = (uint32_t)src[(int64_t)x + k];
                    if (u != 0u) mo_take(bd, bl, wk2, u);
                }
            }
        }
        kd[i] = (uint16_t)bd;
        kl[i] = bl;
    }
}

// one more axis: both sides at step k before k + 1, so that the bound w k^2 <= best d^2 holds for either
template <typename Key>
__device__ __forceinline__ void mo_near_line(int &bd, uint32_t &bl, int w, int r2, int64_t before, int64_t after, Key key_at)
{
    for (int64_t k = 1;; ++k) {
        const int wk2 = w * (int)k * (int)k;
        if (wk2 > min(bd, r2) || (k > before && k > after)) break;
        if (k <= before) key_at(-k, wk2);
        if (k <= after) key_at(k, wk2);
    }
}

__global__ __launch_bounds__(256) void mo_near_y_kernel(uint32_t n, uint32_t H, uint32_t W, int w, int r2,
                                                        const uint16_t *__restrict__ kd, const uint32_t *__restrict__ kl,
                                                        uint16_t *__restrict__ od, uint32_t *__restrict__ ol)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t row = i / W, y = row % H;
        int bd = kd[i];
        uint32_t bl = kl[i];
        if (bd != 0)
            mo_near_line(bd, bl, w, r2, y, (int64_t)H - 1 - y, [&](int64_t s, int wk2) {
                const int64_t q = (int64_t)i + s * (int64_t)W;
                const int d = (int)kd[q] + wk2;
                if (d <= r2) mo_take(bd, bl, d, kl[q]);
            });
        od[i] = (uint16_t)bd;
        ol[i] = bl;
    }
}

// the z pass over the core slices: a labelled voxel keeps its label, a zero voxel takes the nearest label within r2
template <typename T>
__global__ __launch_bounds__(256) void mo_near_z_kernel(uint32_t n, uint32_t HW, int64_t hb, int64_t Z, int w, int r2,
                                                        const uint16_t *__restrict__ kd, const uint32_t *__restrict__ kl,
                                                        T *__restrict__ out)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t ze = (int64_t)(i / HW) + hb, e = (int64_t)i + hb * (int64_t)HW;
        int bd = kd[e];
        uint32_t bl = kl[e];
        if (bd != 0)
            mo_near_line(bd, bl, w, r2, ze, Z - 1 - ze, [&](int64_t s, int wk2) {
                const int64_t q = e + s * (int64_t)HW;
                const int d = (int)kd[q] + wk2;
                if (d <= r2) mo_take(bd, bl, d, kl[q]);
            });
        out[i] = bd <= r2 ? (T)bl : (T)0;
    }
}

// ------------------------------------------------------------------------------------------ entry points
struct MoShape {
    int64_t D, H, W, hb, ha, Z, n_ext, n_core;
};

#define MO_REQUIRE_ARGS(what)                                                                                         \
    do {                                                                                                              \
        EMP_REQUIRE_VOLUME(what);                                                                                     \
        EMP_REQUIRE(hb >= 0 && ha >= 0, what ": bad halo counts (%lld, %lld)", (long long)hb, (long long)ha);         \
        EMP_REQUIRE(D <= 0x7fffffffLL && hb <= 0x7fffffffLL && ha <= 0x7fffffffLL && H <= 0x7fffffffLL / W &&        \
                        (D + hb + ha == 0 || H * W <= 0x7fffffffLL / (D + hb + ha)),                                  \
                    what ": (%lld + %lld + %lld) x %lld x %lld voxels exceed 2^31 - 1; cut the slab into z-blocks",   \
                    (long long)hb, (long long)D, (long long)ha, (long long)H, (long long)W);                          \
        EMP_REQUIRE(az >= 1 && az <= 16 && ay >= 1 && ay <= 16 && ax >= 1 && ax <= 16,                                \
                    what ": sampling (%d, %d, %d) outside 1 .. 16", az, ay, ax);                                      \
        EMP_REQUIRE(D == 0 || lab, what ": null pointer");                                                            \
        EMP_REQUIRE((hb == 0 || below) && (ha == 0 || above), what ": a halo count without its stack");               \
        EMP_REQUIRE(reinterpret_cast<uintptr_t>(lab) % (uintptr_t)item == 0 &&                                        \
                        reinterpret_cast<uintptr_t>(below) % (uintptr_t)item == 0 &&                                  \
                        reinterpret_cast<uintptr_t>(above) % (uintptr_t)item == 0,                                    \
                    what ": misaligned labels");                                                                      \
    } while (0)

#define MO_REQUIRE_R2(what)                                                                                           \
    do {                                                                                                              \
        EMP_REQUIRE(r2 >= 1 && r2 <= 65534, what ": r2 = %d outside 1 .. 65534", r2);                                 \
        EMP_REQUIRE(r2 >= az * az || r2 >= ay * ay || r2 >= ax * ax,                                                  \
                    what ": r2 = %d is below the smallest squared pitch of (%d, %d, %d): the ball is a point", r2, az, \
                    ay, ax);                                                                                          \
    } while (0)

static MoShape mo_shape(int64_t D, int64_t H, int64_t W, int64_t hb, int64_t ha)
{
    MoShape S;
    S.D = D; S.H = H; S.W = W; S.hb = hb; S.ha = ha;
    S.Z = hb + D + ha;
    S.n_ext = S.Z * H * W;
    S.n_core = D * H * W;
    return S;
}

struct MoEdtWork {
    uint16_t *f, *g;
    int64_t total;
};
static MoEdtWork mo_edt_carve(void *work, int64_t n_ext)
{
    if (n_ext < 1) n_ext = 1;
    EmpCarver c(work);
    MoEdtWork L;
    L.f = c.take<uint16_t>(n_ext);
    L.g = c.take<uint16_t>(n_ext);
    L.total = c.bytes();
    return L;
}

struct MoNearWork {
    uint16_t *d0, *d1;
    uint32_t *l0, *l1;
    int64_t total;
};
static MoNearWork mo_near_carve(void *work, int64_t n_ext)
{
    if (n_ext < 1) n_ext = 1;
    EmpCarver c(work);
    MoNearWork L;
    L.d0 = c.take<uint16_t>(n_ext);
    L.d1 = c.take<uint16_t>(n_ext);
    L.l0 = c.take<uint32_t>(n_ext);
    L.l1 = c.take<uint32_t>(n_ext);
    L.total = c.bytes();
    return L;
}

static int64_t mo_work_bytes(int64_t D, int64_t H, int64_t W, int64_t hb, int64_t ha, bool near)
{
    if (D < 0 || H < 1 || W < 1 || hb < 0 || ha < 0 || D > 0x7fffffffLL || hb > 0x7fffffffLL || ha > 0x7fffffffLL ||
        H > 0x7fffffffLL / W || (D + hb + ha > 0 && H * W > 0x7fffffffLL / (D + hb + ha)))
        return -1;
    const int64_t n = (D + hb + ha) * H * W;
    return near ? mo_near_carve(nullptr, n).total : mo_edt_carve(nullptr, n).total;
}
extern "C" int64_t emp_label_edt_work_bytes(int64_t D, int64_t H, int64_t W, int64_t hb, int64_t ha)
{
    return mo_work_bytes(D, H, W, hb, ha, false);
}
extern "C" int64_t emp_label_dilate_work_bytes(int64_t D, int64_t H, int64_t W, int64_t hb, int64_t ha)
{
    return mo_work_bytes(D, H, W, hb, ha, true);
}

template <typename T, bool ERODE, bool ALL = false>
static int mo_edt_launch(const MoShape &S, const void *lab, const void *below, const void *above, int az, int ay, int ax,
                         int cap, const MoEdtWork &L, void *out, hipStream_t st)
{
    MoVol<T> vol = {reinterpret_cast<const T *>(below), reinterpret_cast<const T *>(lab),
                    reinterpret_cast<const T *>(above), S.hb, S.D, S.ha, S.H * S.W};
    const int64_t rows = S.Z * S.H;
    EMP_LAUNCH((mo_edt_rows_kernel<T>), emp_grid(rows * 64, 256, 16384), 256, st, vol, rows, S.H, S.W, ax * ax, cap, L.f);
    EMP_LAUNCH((mo_edt_y_kernel<T>), emp_grid(S.n_ext, 256, 16384), 256, st, vol, (uint32_t)S.n_ext, (uint32_t)S.H,
               (uint32_t)S.W, ay * ay, L.f, L.g);
    const int64_t n_out = ALL ? S.n_ext : S.n_core;
    EMP_LAUNCH((mo_edt_z_kernel<T, ERODE, ALL>), emp_grid(n_out, 256, 16384), 256, st, vol, (uint32_t)n_out,
               (uint32_t)(S.H * S.W), az * az, cap, L.g, out);
    return EMP_OK;
}

static int mo_edt_run(const char *what, const void *lab, int item, const MoShape &S, const void *below, const void *above,
                      int az, int ay, int ax, int cap, void *work, int64_t work_bytes, void *out, bool erode, void *stream)
{
    if (S.D == 0) return EMP_OK;
    EMP_REQUIRE(work && out, "%s: null pointer", what);
    EMP_REQUIRE(out != lab, "%s: the output must not be the input", what);
    MoEdtWork L = mo_edt_carve(work, S.n_ext);
    EMP_REQUIRE(work_bytes >= L.total, "%s: workspace too small (%lld < %lld)", what, (long long)work_bytes,
                (long long)L.total);
    hipStream_t st = emp_stream(stream);
    if (item == 4)
        return erode ? mo_edt_launch<uint32_t, true>(S, lab, below, above, az, ay, ax, cap, L, out, st)
                     : mo_edt_launch<uint32_t, false>(S, lab, below, above, az, ay, ax, cap, L, out, st);
    return erode ? mo_edt_launch<uint8_t, true>(S, lab, below, above, az, ay, ax, cap, L, out, st)
                 : mo_edt_launch<uint8_t, false>(S, lab, below, above, az, ay, ax, cap, L, out, st);
}

extern "C" int emp_label_edt(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below, int64_t hb,
                             const void *above, int64_t ha, int az, int ay, int ax, int cap, void *work,
                             int64_t work_bytes, uint16_t *out, void *stream)
{
    MO_REQUIRE_ARGS("label_edt");
    EMP_REQUIRE(cap >= 1 && cap <= 65535, "label_edt: cap = %d outside 1 .. 65535", cap);
    return mo_edt_run("label_edt", lab, item, mo_shape(D, H, W, hb, ha), below, above, az, ay, ax, cap, work, work_bytes,
                      out, false, stream);
}

// the x pass writes `d2`, the y pass reads it and writes `tmp`, the z pass reads `tmp` and writes `d2`
int emp_label_edt_extended(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below, int64_t hb,
                           const void *above, int64_t ha, int az, int ay, int ax, int cap, uint16_t *d2, uint16_t *tmp,
                           void *stream)
{
    MO_REQUIRE_ARGS("label_edt_extended");
    EMP_REQUIRE(cap >= 1 && cap <= 65535, "label_edt_extended: cap = %d outside 1 .. 65535", cap);
    const MoShape S = mo_shape(D, H, W, hb, ha);
    if (S.n_ext == 0) return EMP_OK;
    EMP_REQUIRE(d2 && tmp, "label_edt_extended: null pointer");
    MoEdtWork L;
    L.f = d2;
    L.g = tmp;
    L.total = 0;
    hipStream_t st = emp_stream(stream);
    return item == 4 ? mo_edt_launch<uint32_t, false, true>(S, lab, below, above, az, ay, ax, cap, L, d2, st)
                     : mo_edt_launch<uint8_t, false, true>(S, lab, below, above, az, ay, ax, cap, L, d2, st);
}

extern "C" int emp_label_erode(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below, int64_t hb,
                               const void *above, int64_t ha, int az, int ay, int ax, int r2, void *work,
                               int64_t work_bytes, void *out, void *stream)
{
    MO_REQUIRE_ARGS("label_erode");
    MO_REQUIRE_R2("label_erode");
    return mo_edt_run("label_erode", lab, item, mo_shape(D, H, W, hb, ha), below, above, az, ay, ax, r2 + 1, work,
                      work_bytes, out, true, stream);
}

template <typename T>
static int mo_near_launch(const MoShape &S, const void *lab, const void *below, const void *above, int az, int ay, int ax,
                          int r2, const MoNearWork &L, void *out, hipStream_t st)
{
    MoVol<T> vol = {reinterpret_cast<const T *>(below), reinterpret_cast<const T *>(lab),
                    reinterpret_cast<const T *>(above), S.hb, S.D, S.ha, S.H * S.W};
    const int grid = emp_grid(S.n_ext, 256, 16384);
    EMP_LAUNCH((mo_near_x_kernel<T>), grid, 256, st, vol, (uint32_t)S.n_ext, (uint32_t)S.H, (uint32_t)S.W, ax * ax, r2,
               L.d0, L.l0);
    EMP_LAUNCH(mo_near_y_kernel, grid, 256, st, (uint32_t)S.n_ext, (uint32_t)S.H, (uint32_t)S.W, ay * ay, r2, L.d0, L.l0,
               L.d1, L.l1);
    EMP_LAUNCH((mo_near_z_kernel<T>), emp_grid(S.n_core, 256, 16384), 256, st, (uint32_t)S.n_core, (uint32_t)(S.H * S.W),
               S.hb, S.Z, az * az, r2, L.d1, L.l1, reinterpret_cast<T *>(out));
    return EMP_OK;
}

extern "C" int emp_label_dilate(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below, int64_t hb,
                                const void *above, int64_t ha, int az, int ay, int ax, int r2, void *work,
                                int64_t work_bytes, void *out, void *stream)
{
    MO_REQUIRE_ARGS("label_dilate");
    MO_REQUIRE_R2("label_dilate");
    if (D == 0) return EMP_OK;
    EMP_REQUIRE(work && out, "label_dilate: null pointer");
    EMP_REQUIRE(out != lab, "label_dilate: the output must not be the input");
    const MoShape S = mo_shape(D, H, W, hb, ha);
    MoNearWork L = mo_near_carve(work, S.n_ext);
    EMP_REQUIRE(work_bytes >= L.total, "label_dilate: workspace too small (%lld < %lld)", (long long)work_bytes,
                (long long)L.total);
    hipStream_t st = emp_stream(stream);
    return item == 4 ? mo_near_launch<uint32_t>(S, lab, below, above, az, ay, ax, r2, L, out, st)
                     : mo_near_launch<uint8_t>(S, lab, below, above, az, ay, ax, r2, L, out, st);
}
