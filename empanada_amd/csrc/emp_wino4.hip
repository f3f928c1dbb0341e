// D5d: Winograd F(4x4, 3x3) convolution + BatchNorm (+ ReLU) in ONE kernel for layer1's conv2 (64 -> 64), the only width
// pair emp_wino4_fused_eligible enables.  128 -> 128 (layer2's conv2) is instantiated and tested through fused=True, but
// gains only 4-9 % on the bench's shape and stays on the three calls (profiles/wino4_fused.md).  gfx950 only.
//
// Why.  The three-call path (emp_wino4_input_transform, emp_gemm_nt_batched x 36, emp_wino4_output_transform) passes
// V (36, T, Cin) and Mw (36, T, Cout) through memory: about 11x the activation's bytes where the convolution needs 2x,
// and at these widths that traffic, not the matrix work, is the running time.  Here V lives in LDS one 16-channel slab at
// a time and M stays in the accumulators from the first MFMA to the output transform.
//   * grid = 256 persistent 512-thread blocks, one per CU of the MI355X (an assumption about the device, like the other
//     persistent launchers here; another CU count only changes the balance, the items are strided by gridDim); a work item is (group of 32 consecutive tiles, group of 64 couts).
//     A block's tile groups come from ONE XCD's contiguous range of the tile table, so that the patch rows neighbouring
//     tile rows share come out of that XCD's L2 (as in wino4_input_kernel); the cout groups of a tile group run back to
//     back on the same block and recompute the V slabs (the patch is then in L1 / L2).
//   * K loop over 16-channel slabs.  Thread (tile, channel) gathers its 36 patch pixels, applies B^T d B with the
//     operations of wino4_input_kernel and writes 36 values to the LDS slab Vs[position][channel][tile], rows padded to
//     34 floats: the transform's writes and the MFMA operand reads are both conflict-free.  The NEXT slab's patch loads
//     are issued before the current slab's MFMAs and consumed after them (an item's first slab: before its predecessor's
//     column step and stores).
//   * 36 x 32 x 64 accumulators are 288 registers per lane of four waves -- more than the 256 AGPRs, and the compiler
//     spills.  So EIGHT waves, two per SIMD with 256 registers each: wave (h, w) owns couts 16 w .. 16 w + 15 of the cout
//     group, both 16-tile row tiles and the 18 positions of the patch COLUMNS 3 h .. 3 h + 2 (144 accumulator registers):
//     v_mfma_f32_16x16x4_f32 with A = V from LDS (one ds_read_b32 per MFMA) and B = U straight from global memory / L2
//     (one float4 per lane, position and slab, the halves of the wave trading registers; no wave repeats another's U
//     loads; U is re-read once per work item).
//   * after the last slab lane (cout c, quarter q) of wave (h, w) holds M[a][3 h + bb] of the tiles 4 q .. 4 q + 3 of both
//     row tiles.  The output transform's row step s = A^T m works on one column at a time, so each wave applies it to its
//     own columns in registers; then the two waves of a pair swap halves through LDS (48 values per lane: wave h gets the
//     other three columns of row tile h) and each finishes 4 tiles per lane: column step, epilogue, store -- the
//     operations of wino4_output_kernel; a 16-lane group stores 64 contiguous bytes per pixel.
// Summation order per M value: one fma chain from +0 over 16-channel slabs ascending, inside a slab c, c + 8 for
// c = 0..7 -- step j of a slab feeds channels 2j, 2j + 8, 2j + 1, 2j + 9 to k = 0..3 of one MFMA, which is a chain over
// its four k.  That is the order of emp_gemm_nt_batched at K-slab 16, so the result is bit-identical to the three-call
// path wherever the plan's slab is 16 (emp_conv_k_slab(T, Cout, 36, 0)); oracle/dense.py::wino4_conv_bn_act(slab=16)
// describes both.
#include "emp_common.h"
#include "emp_wino4.h"
#include <stdlib.h>
#include <type_traits>

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define WF_THREADS 512
#define WF_G 32                    // tiles per work item: two 16-row MFMA tiles
#define WF_S 16                    // K-slab
#define WF_RS 34                   // LDS row (floats): 32 tiles + 2, so that channels c and c + 8 sit 16 banks apart
#define WF_PS (WF_S * WF_RS)       // floats per position
#define WF_PF 3                    // positions whose U fragments are requested ahead of their MFMAs
#define WF_XCH (WF_THREADS * 48)   // floats the wave pairs swap in the epilogue
#define WF_T_MIN 3136              // smallest measured T at which the kernel is still ahead (a tie at 2 304: profiles/wino4_fused.md)

struct WfGeom {
    const float *x, *U, *scale, *shift;
    const int32_t *tiles;
    float *out;
    int64_t T, out_ps;
    int H, W, dil, groups;         // groups = ceil(T / 32)
};

template <int CIN, int COUT, bool RELU>
__global__ __launch_bounds__(WF_THREADS, 2) void wino4_fused_kernel(WfGeom g)
{
    constexpr int KS = CIN / WF_S;                     // slabs
    constexpr int CG = COUT / 64;                      // cout groups
    __shared__ __attribute__((aligned(16))) float Vs[36 * WF_PS > WF_XCH ? 36 * WF_PS : WF_XCH];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tl = tid >> 4, ch = tid & 15;            // transform role: tile of the group, channel of the slab
    const int ci = lane & 15, q = lane >> 4;           // MFMA role: A row (tile) / B, C column (cout); k index / row quarter
    const int odd = q >> 1;                            // k = 0..3 of step j takes channels 2j, 2j + 8, 2j + 1, 2j + 9
    const int h = wave >> 2, w4 = wave & 3;            // patch columns 3 h .. 3 h + 2; couts 16 w4 .. + 15

    // the block's work items: tile groups lo + slot, lo + slot + per, ... below hi of its XCD's range, CG cout groups each
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per = gridDim.x >> 3;
    const int lo = (int)((int64_t)g.groups * xcd / 8), hi = (int)((int64_t)g.groups * (xcd + 1) / 8);
    const int n_items = slot < hi - lo ? ((hi - lo - slot + per - 1) / per) * CG : 0;

    // patch pixels of the thread's tile, channel 16 s + ch.  Branch-free, so that the loads stay in flight across the
    // MFMAs: a pixel outside the image (or of a tile past T) is loaded from the clamped position and replaced by 0 in
    // transform(), by the returned mask: bit a = row a inside, bit 6 + b = column b inside (0 for a tile past T)
    auto load_raw = [&](int item, int s, v1 (&raw)[6][6]) -> int {
        const int64_t t = (int64_t)(lo + slot + (item / CG) * per) * WF_G + tl;
        const bool live = t < g.T;
        const int64_t tc = live ? t : g.T - 1;
        const int n = g.tiles[3 * tc], by = g.tiles[3 * tc + 1], bx = g.tiles[3 * tc + 2];
        // byte offsets from the uniform base fit 32 bits (launcher), so that the 36 loads need one address register each
        const uint32_t src = 4u * ((uint32_t)n * (uint32_t)(g.H * g.W * CIN) + (uint32_t)(WF_S * s + ch));
        const char *xb = reinterpret_cast<const char *>(g.x);
        int mask = 0;
        uint32_t xo[6];
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const int xx = bx + b * g.dil;
            if (live && xx >= 0 && xx < g.W) mask |= 64 << b;
            xo[b] = 4u * (uint32_t)(min(max(xx, 0), g.W - 1) * CIN);
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const int yy = by + a * g.dil;
            if (live && yy >= 0 && yy < g.H) mask |= 1 << a;
            const uint32_t row = src + 4u * (uint32_t)(min(max(yy, 0), g.H - 1) * (g.W * CIN));
#pragma unroll
            for (int b = 0; b < 6; ++b) raw[a][b] = {*reinterpret_cast<const float *>(xb + (row + xo[b]))};
        }
        return mask;
    };
    // V = B^T d B (columns, then rows) of the thread's (tile, channel) -> Vs[position][channel][tile]
    auto transform = [&](const v1 (&raw)[6][6], int mask) {
        v1 tt[6][6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            v1 d[6];
#pragma unroll
            for (int b = 0; b < 6; ++b) d[b] = {(mask >> a & 1) && (mask >> (6 + b) & 1) ? raw[a][b].x : 0.f};
            wino4_bt(d, tt[a]);
        }
        float *dst = &Vs[ch * WF_RS + tl];
#pragma unroll
        for (int v = 0; v < 6; ++v) {
            v1 col[6], r[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) col[a] = tt[a][v];
            wino4_bt(col, r);
#pragma unroll
            for (int u = 0; u < 6; ++u) dst[(u * 6 + v) * WF_PS] = r[u].x;
        }
    };

    // the lane's A element of step 0, row tile 0, and its 4 channels of slab 0, cout group 0 -- both of position 3 h
    const float *Al = &Vs[3 * h * WF_PS + (8 * (q & 1) + odd) * WF_RS + ci];
    const float *Ul = g.U + ((int64_t)3 * h * COUT + 16 * w4 + ci) * CIN + 8 * (q & 1) + 4 * odd;

    v1 raw[6][6];
    int mask = 0;
    if (n_items > 0) mask = load_raw(0, 0, raw);
    for (int item = 0; item < n_items; ++item) {
        const int cg = item % CG;
        f32x4 acc[18][2];                              // local position lp = 3 a + bb: position 6 a + 3 h + bb
#pragma unroll
        for (int lp = 0; lp < 18; ++lp)
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) acc[lp][rt] = {0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
        for (int s = 0; s < KS; ++s) {
            transform(raw, mask);
            __syncthreads();
            // U fragments of the first WF_PF positions, then the next slab's patch (slab 0 of the next item: see the epilogue)
            const float *up = Ul + (int64_t)cg * 64 * CIN + WF_S * s;
            auto uoff = [](int lp) { return (int64_t)((lp / 3) * 6 + lp % 3) * COUT * CIN; };
            float4 bq[WF_PF];
#pragma unroll
            for (int lp = 0; lp < WF_PF; ++lp) bq[lp] = *reinterpret_cast<const float4 *>(up + uoff(lp));
            if (s + 1 < KS) mask = load_raw(item, s + 1, raw);
#pragma unroll
            for (int lp = 0; lp < 18; ++lp) {
                float4 c = bq[lp % WF_PF];
                // (opaque here, where the fragment is consumed: otherwise the swaps below are scheduled right behind the
                // loads and wait for them at once)
                asm volatile("" : "+v"(c.x), "+v"(c.y), "+v"(c.z), "+v"(c.w));
                if (lp + WF_PF < 18) bq[lp % WF_PF] = *reinterpret_cast<const float4 *>(up + uoff(lp + WF_PF));
                // lanes 0-31 hold channels 0..3 of their half-slab, lanes 32-63 channels 4..7; steps j = 0..3 want channels
                // 0, 2, 4, 6 in lanes 0-31 and 1, 3, 5, 7 in lanes 32-63: v_permlane32_swap (x, y) and (z, w)
                const auto s0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(c.x), __float_as_uint(c.y), false, false);
                const auto s1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(c.z), __float_as_uint(c.w), false, false);
                const float bv[4] = {__uint_as_float(s0[0]), __uint_as_float(s1[0]), __uint_as_float(s0[1]), __uint_as_float(s1[1])};
                const float *ap = Al + ((lp / 3) * 6 + lp % 3) * WF_PS;
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt)
                        acc[lp][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[2 * j * WF_RS + 16 * rt], bv[j], acc[lp][rt], 0, 0, 0);
            }
            __syncthreads();                           // every wave is done with this slab of Vs
        }

        // ---- output transform.  Register r of acc[3 a + bb][rt] = M[a][3 h + bb] of tile 16 rt + 4 q + r, cout co.
        // rows: s[a'][b] = A^T over a, per column b; row tile h stays (keep), row tile 1 - h goes to the partner wave
        const int co = cg * 64 + 16 * w4 + ci;
        // (column by column, the partner's row tile first: the accumulators are released as early as possible)
        float keep[4][3][4];                           // [r][bb][a']
        float *xw = &Vs[((wave ^ 4) * 48) * 64 + lane];
        const float *xr = &Vs[(wave * 48) * 64 + lane];
        auto rows = [&](auto rtc, auto sendc) {
            constexpr int rt = decltype(rtc)::value;
            constexpr bool send = decltype(sendc)::value;
#pragma unroll
            for (int bb = 0; bb < 3; ++bb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v1 m[6], rr[4];
#pragma unroll
                    for (int a = 0; a < 6; ++a) m[a] = {acc[3 * a + bb][rt][r]};
                    wino4_at(m, rr);
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        if (send) xw[((r * 3 + bb) * 4 + a) * 64] = rr[a].x;
                        else keep[r][bb][a] = rr[a].x;
                    }
                }
        };
        using std::integral_constant;
        if (h == 0) {
            rows(integral_constant<int, 1>(), integral_constant<bool, true>());
            rows(integral_constant<int, 0>(), integral_constant<bool, false>());
        } else {
            rows(integral_constant<int, 0>(), integral_constant<bool, true>());
            rows(integral_constant<int, 1>(), integral_constant<bool, false>());
        }
        // slab 0 of the next item's patch, now that the accumulators are free; it lands during the column step and the stores
        if (item + 1 < n_items) mask = load_raw(item + 1, 0, raw);
        __syncthreads();

        // columns: y = s A, then the epilogue, for the lane's 4 tiles of row tile h
        const float sc = g.scale[co], sh = g.shift[co];
        const int64_t t0 = (int64_t)(lo + slot + (item / CG) * per) * WF_G + 16 * h + 4 * q;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t t = t0 + r;
            if (t < g.T) {
                const int n = g.tiles[3 * t], oy = g.tiles[3 * t + 1] + g.dil, ox = g.tiles[3 * t + 2] + g.dil;
                float *dst = g.out + (int64_t)n * g.H * g.W * g.out_ps + co;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    v1 sm[6], yv[4];
#pragma unroll
                    for (int bb = 0; bb < 3; ++bb) {
                        const float got = xr[((r * 3 + bb) * 4 + a) * 64];
                        sm[bb] = {h ? got : keep[r][bb][a]};
                        sm[3 + bb] = {h ? keep[r][bb][a] : got};
                    }
                    wino4_at(sm, yv);
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int yy = oy + a * g.dil, xx = ox + b * g.dil;
                        if (yy < g.H && xx < g.W) {
                            float v = __fadd_rn(__fmul_rn(yv[b].x, sc), sh);
                            if (RELU) v = fmaxf(v, 0.f);
                            dst[((int64_t)yy * g.W + xx) * g.out_ps] = v;
                        }
                    }
                }
            }
        }
        __syncthreads();                               // (the next item's transform overwrites what the partner reads)
    }
}

static bool wf_off()
{
    static const char *off = getenv("EMP_WINO4_NO_FUSED");     // experiments only (A/B against the three-call path)
    return off && off[0] == '1';
}

// the widths the kernel is built for, and the summation order it is bit-identical at
static bool wf_shape_ok(int64_t T, int Cin, int Cout)
{
    // (a tile has at most 16 pixels, N H W <= 16 T: the bound keeps the activation's byte offsets below 2^32)
    return ((Cin == 64 && Cout == 64) || (Cin == 128 && Cout == 128)) && T > 0 && 16 * T * Cin < (1LL << 30) &&
           emp_conv_k_slab(T, Cout, 36, 0) == WF_S;
}

// 1 = _hip.wino4_conv_bn_act takes the one-kernel path: an enabled width pair (profiles/wino4_fused.md), scale AND shift,
// the K-slab 16 order, and at least the measured minimum of tiles
extern "C" int emp_wino4_fused_eligible(int64_t T, int Cin, int Cout, int has_scale_shift)
{
    if (wf_off() || !has_scale_shift) return 0;
    if (!(Cin == 64 && Cout == 64)) return 0;          // 128 -> 128 is built and tested, but did not win clearly: record only
    return wf_shape_ok(T, Cin, Cout) && T >= WF_T_MIN;
}

extern "C" int emp_wino4_conv_bn_act_nhwc(const float *x, int N, int H, int W, int Cin, int dil, const int32_t *tiles,
                                          int64_t T, const float *U, int Cout, const float *scale, const float *shift,
                                          int relu, float *out, int64_t out_pixel_stride, void *stream)
{
    EMP_REQUIRE(x && tiles && U && scale && shift && out, "wino4_conv: null pointer (scale and shift are required)");
    EMP_REQUIRE(N > 0 && H > 0 && W > 0 && dil >= 1 && T >= 0, "wino4_conv: bad shape");
    if (out_pixel_stride == 0) out_pixel_stride = Cout;
    EMP_REQUIRE(out_pixel_stride >= Cout, "wino4_conv: bad pixel stride");
    EMP_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(U)) & 15) == 0 &&
                (reinterpret_cast<uintptr_t>(out) & 3) == 0, "wino4_conv: alignment");
    if (T == 0) return EMP_OK;
    EMP_REQUIRE(wf_shape_ok(T, Cin, Cout), "wino4_conv: 64 -> 64 or 128 -> 128 with the K-slab 16 plan only (T = %lld, %d -> %d)",
                (long long)T, Cin, Cout);
    EMP_REQUIRE((int64_t)N * H * W * Cin < (1LL << 30) && T < (1LL << 31) - WF_G, "wino4_conv: activation too large for 32-bit byte offsets");
    WfGeom g;
    g.x = x; g.U = U; g.scale = scale; g.shift = shift; g.tiles = tiles; g.out = out;
    g.T = T; g.out_ps = out_pixel_stride; g.H = H; g.W = W; g.dil = dil;
    g.groups = (int)emp_cdiv(T, WF_G);
    hipStream_t st = emp_stream(stream);
    const dim3 grid(256), block(WF_THREADS);           // one block per CU of the MI355X (256, not queried); a multiple of 8: see the work items
    if (Cin == 64) {
        if (relu) hipLaunchKernelGGL((wino4_fused_kernel<64, 64, true>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((wino4_fused_kernel<64, 64, false>), grid, block, 0, st, g);
    } else {
        if (relu) hipLaunchKernelGGL((wino4_fused_kernel<128, 128, true>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((wino4_fused_kernel<128, 128, false>), grid, block, 0, st, g);
    }
    EMP_CHECK_LAUNCH("emp_wino4_conv_bn_act_nhwc");
    return EMP_OK;
}
