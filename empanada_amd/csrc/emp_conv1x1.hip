// D4b: weight-stationary 1x1 convolution + BatchNorm (+ residual) (+ ReLU) for the SHORT-K pointwise layers of the
// ResNet bottleneck (layer1 / layer2: conv3 64 -> 256 and 128 -> 512 with the identity added, the 64 -> 256 shortcut
// projection; further shapes at the end of this comment).  gfx950 only.
//
// Why a second kernel.  These layers move 2.3-4.6 KB per pixel for 33-131 kFLOP: 14-28 flop per byte, at or below the
// ridge of the fp32 matrix pipe (157 TF/s / 6.3 TB/s = 25).  The tiled implicit-GEMM kernel (emp_conv.hip) spends a
// block's life in prologue and epilogue there -- 2 or 4 K-slabs between staging 64 KB of operands and draining 64 KB
// of output through LDS -- and reaches 3.6-3.9 TB/s on layer1, 2.7 TB/s on layer2 (profiles/r2_res1x1_variants).
// Here nothing but the weights touches LDS, and they are staged ONCE per block:
//   * grid = one 256-thread block per CU, persistent; a block owns 128 couts (blockIdx -> (pixel block, cout group),
//     the cout groups of one pixel block on the same XCD so that the activations they share come out of that XCD's
//     L2) and keeps their 128 x Cin weights in LDS for its whole life (34-68 KB);
//   * a wave owns a 32-pixel x 128-cout tile per step: the A operand (32 pixels x Cin) goes from global memory
//     STRAIGHT INTO THE MFMA SOURCE REGISTERS -- with the K order "k-step j consumes channels j (lanes 0-31) and
//     32 + j (lanes 32-63) of a 64-channel slab" lane (r, h) needs exactly the contiguous 128 bytes
//     x[pixel r][64 s + 32 h .. + 32) -- no LDS staging, no barrier anywhere in the loop;
//   * the four 32 x 32 accumulator tiles of a wave cover couts n0 + 4 c + j (tile j, column c): the weights are
//     staged in that permuted row order, so that in the epilogue lane c holds FOUR CONSECUTIVE couts of a pixel in the
//     same register index of its four tiles -- residual loads and output stores are float4 per lane, 512 contiguous
//     bytes per half-wave, straight from / to the accumulators (no LDS transpose);
//   * ONE wave per SIMD with the whole 512-entry register file (two waves of 256 spill), software-pipelined over two
//     register sets: a tile's residual and the NEXT tile's activations are requested a whole matrix phase (128-256
//     MFMAs, 3-7 us) before they are consumed (~100 KB in flight per CU), and the epilogue of tile i - 1 is issued
//     in the shadow of tile i's MFMAs (two accumulator sets).
// Summation order per output: one fmaf chain from +0 over 64-channel slabs ascending, inside a slab j = 0..31:
// channel j, then channel 32 + j -- the order of emp_conv_bn_act_nhwc with a K-slab of 64 (emp_conv_k_slab_geom);
// oracle/dense.py::conv_bn_act_nhwc(slab=64) reproduces it bit for bit.
//
// The same kernel, with the K-slab, the cout-group width and the pixels per wave step as template parameters, also takes
// the short-K launches the tiled kernel is worst at (profiles/ws_shapes.md): the bottleneck's conv1 (256 -> 64, 64 -> 64,
// 256 -> 128 with BatchNorm + ReLU) and the batched GEMM behind emp_gemm_nt_batched with K and N in {64, 128} (the
// Winograd F(4x4,3x3) GEMMs of layer1 / layer2).  THOSE sum in the tiled kernel's own order -- slabs of S = 16 channels,
// inside a slab c, c + S/2 for c = 0..S/2-1 -- so their results do not depend on which kernel ran.
#include "emp_common.h"
#include <stdlib.h>
#include <atomic>
#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));
template <int V> using IC = std::integral_constant<int, V>;

#define PW_THREADS 256
#define PW_ROWS 32                 // pixels per 32 x 32 MFMA tile
#define PW_MIN_ROWS 65536          // 64-slab shapes: fewest pixels worth the persistent grid
#define PW_MIN_ROWS_PLAN 262144    // plan-order shapes and the batched GEMM: at least eight 32-row tiles per wave (256 CUs
                                   // x 4 waves), so that the pipeline's fill and drain are a small part of a wave's life

struct PwGeom {
    const float *x, *w, *scale, *shift, *res;
    float *out;
    int64_t M, out_ps, res_ps;
    int Cin, Cout, relu, groups, pix_blocks;
    int batch;                     // GEMM form: entries per launch; x, w and out advance by x_bs, w_bs, out_bs per entry
    int64_t x_bs, w_bs, out_bs;
};

// KS:   Cin / 64.
// S:    K-slab of the summation order: the k-step j of slab s consumes channels S s + j (lanes 0-31) and S s + S/2 + j
//       (lanes 32-63), so lane (r, h) reads the S/2 contiguous channels [S s + h S/2, S s + h S/2 + S/2) of slab s --
//       128 contiguous bytes at S = 64, 32-byte pieces of the same row at S = 16 -- and the weight fragments come from the
//       matching LDS columns.  S = 64 for the conv3 / shortcut shapes, else the slab of the tiled kernel's plan
//       (emp_conv_k_slab*), so that for those shapes the result does not depend on which kernel ran.
// CT:   32-wide cout tiles of a block: 4 (128 couts, a lane holds 4 consecutive couts, float4 epilogue) or 2 (64 couts,
//       a lane holds 2 consecutive couts; a half-wave store still covers a whole 256-byte pixel row).
// PT:   32-pixel tiles per wave step (2 where the A registers allow it: more bytes in flight per wave for the layers
//       with the fewest flops per byte).
// GEMM: batched C_b = A_b B_b^T with the identity epilogue; a block takes a contiguous range of the launch's
//       (entry, tile) sequence and re-stages the weights where the range crosses into the next entry.
// MODE: 0  the forms above.
//       1  (RES) the Cin = 256 form: ONE residual register set, and the activations through a ring of four 32-channel
//          slabs (64 registers) refilled slab by slab behind eight fenced eighths of a tile's MFMAs, instead of two whole
//          activation sets (2 x 128 registers), which do not fit next to the accumulators' copies the epilogue needs; the
//          wave index is a scalar.  Described where it is implemented, in run() below.
template <int KS, int S, int CT, int PT, bool GEMM, bool RES, bool RELU, int MODE = 0>
__global__ __launch_bounds__(PW_THREADS, 1) void conv1x1_ws_kernel(PwGeom g)
{
    static_assert(MODE == 0 || RES, "MODE 1 is a residual form");
    constexpr int CIN = 64 * KS;
    constexpr int LD = CIN + 4;                        // LDS row (floats): 16 lanes x 16 B cover all 64 banks once
    constexpr int BN = 32 * CT;                        // couts per block
    constexpr int NQ = CIN / 8;                        // float4 pieces of A per lane and pixel
    constexpr int QS = S / 8;                          // of which per slab
    constexpr int ROWS = PW_ROWS * PT;                 // pixels per wave step
    static_assert(!RES || (CT == 4 && PT == 1 && !GEMM), "residual: 128-cout groups of the convolution form only");
    static_assert(S == 16 || S == 32 || S == 64, "K-slab");
    __shared__ __attribute__((aligned(16))) float Bs[BN * LD];

    // blockIdx -> (pixel block pb, cout group gi): consecutive hardware block ids go to different XCDs; the cout
    // groups of one pixel block take consecutive slots of ONE XCD
    const int bid = blockIdx.x;
    const int xcd = bid & 7, slot = bid >> 3;
    const int per_xcd = g.pix_blocks >> 3;             // pixel blocks per XCD (pix_blocks is a multiple of 8)
    const int gi = slot % g.groups;
    const int pb = xcd * per_xcd + slot / g.groups;
    const int n0 = GEMM ? 0 : gi * BN;
    const int tid = threadIdx.x;
    const float *xb = g.x, *wb = g.w;                  // the current batch entry's operands (GEMM form: they move)
    float *ob = g.out;

    // weights of couts n0 + CT c + j  ->  LDS row j * 32 + c
    auto stage = [&]() {
        for (int idx = tid; idx < BN * (CIN / 4); idx += PW_THREADS) {
            const int rr = idx / (CIN / 4), k4 = idx - rr * (CIN / 4);
            const int cw = n0 + CT * (rr & 31) + (rr >> 5);
            *reinterpret_cast<float4 *>(&Bs[rr * LD + 4 * k4]) = *reinterpret_cast<const float4 *>(wb + (int64_t)cw * CIN + 4 * k4);
        }
        __syncthreads();
    };

    // (MODE 1: the wave index as a scalar, so that tile indices, row bases and the tile loop's branch live in scalar
    // registers and a lane's addresses are a scalar base plus ONE loop-invariant 32-bit lane offset -- 64-bit per-row
    // addresses in vector registers are what these variants have no room for)
    const int wave = MODE != 0 ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6, lane = tid & 63;
    const int r = lane & 31, hh = lane >> 5;
    const int co = n0 + CT * r;                        // the lane's CT consecutive couts
    float sc[CT], sh[CT];                              // scale and shift are both present (eligibility)
    if constexpr (!GEMM) {
        if constexpr (CT == 4) {
            { const float4 t = *reinterpret_cast<const float4 *>(g.scale + co); sc[0] = t.x; sc[1] = t.y; sc[2] = t.z; sc[3] = t.w; }
            { const float4 t = *reinterpret_cast<const float4 *>(g.shift + co); sh[0] = t.x; sh[1] = t.y; sh[2] = t.z; sh[3] = t.w; }
        } else {
            { const float2 t = *reinterpret_cast<const float2 *>(g.scale + co); sc[0] = t.x; sc[1] = t.y; }
            { const float2 t = *reinterpret_cast<const float2 *>(g.shift + co); sh[0] = t.x; sh[1] = t.y; }
        }
    }

    const int64_t n_tiles = (g.M + ROWS - 1) / ROWS;
    const int64_t n_full = g.M / ROWS;
    const float *Bl = &Bs[r * LD + hh * (S / 2)];      // the lane's row of tile 0, its half of a slab
    const int64_t ops = GEMM ? (int64_t)BN : g.out_ps; // (GEMM form: C rows are dense, so the epilogue's row offsets are immediates)
    const unsigned a_lane = r * CIN + hh * (S / 2);    // MODE 1: the lane's part of an activation, residual, output address
    const unsigned r_lane = (unsigned)(4 * hh * g.res_ps + co), o_lane = (unsigned)(4 * hh * ops + co);   // (launcher: strides < 2^24)

    // ---- the pieces of a tile's life --------------------------------------------------------------------------
    // A = S/2 contiguous channels per lane and slab; piece i of a lane is slab i / QS, float4 i % QS of its half
    auto load_a = [&](int64_t t, float4 (&a)[PT][NQ], const float *base) {
#pragma unroll
        for (int p = 0; p < PT; ++p) {
            const int64_t pa = t * ROWS + PW_ROWS * p + r;     // (only full tiles come through here)
            const float *ap = base + pa * CIN + hh * (S / 2);
#pragma unroll
            for (int i = 0; i < NQ; ++i) a[p][i] = *reinterpret_cast<const float4 *>(ap + S * (i / QS) + 4 * (i % QS));
        }
    };
    // residual of the lane's 16 (pixel, 4 couts) outputs
    auto load_rs = [&](int64_t t, float4 (&rs)[RES ? 16 : 1]) {
        if constexpr (MODE == 1) {
            const float *rp = g.res + t * ROWS * g.res_ps;
#pragma unroll
            for (int q = 0; q < 16; ++q)
                rs[q] = *reinterpret_cast<const float4 *>(rp + (int64_t)((q & 3) + 8 * (q >> 2)) * g.res_ps + r_lane);
        } else if constexpr (RES) {
            const float *rp = g.res + (t * ROWS + 4 * hh) * g.res_ps + co;
#pragma unroll
            for (int q = 0; q < 16; ++q)
                rs[q] = *reinterpret_cast<const float4 *>(rp + (int64_t)((q & 3) + 8 * (q >> 2)) * g.res_ps);
        }
    };
    // (pieces [i_lo, i_hi) of the K range; the accumulators start from +0 at piece 0; `a` holds piece i at i - a_off)
    auto mma = [&](f32x16 (&acc)[PT * CT], const auto &a, auto i_lo_c, auto i_hi_c, auto a_off_c) {
        constexpr int i_lo = decltype(i_lo_c)::value, i_hi = decltype(i_hi_c)::value;
        constexpr int a_off = decltype(a_off_c)::value;
        if constexpr (i_lo == 0) {
#pragma unroll
            for (int j = 0; j < PT * CT; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
        }
        // the weight fragments do not depend on the tile: without this the compiler hoists all CT * NQ float4 LDS reads
        // of a lane out of the tile loop (512+ registers) -- the address is made opaque once per tile instead
        int opaque = 0;
        asm volatile("" : "+v"(opaque));               // (an offset, not the pointer: the LDS address space must survive)
        const float *Bt = Bl + opaque;
#pragma unroll
        for (int i = i_lo; i < i_hi; ++i) {
            float4 b[CT];
#pragma unroll
            for (int j = 0; j < CT; ++j) b[j] = *reinterpret_cast<const float4 *>(Bt + j * 32 * LD + S * (i / QS) + 4 * (i % QS));
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int p = 0; p < PT; ++p) {
                    const float av = e == 0 ? a[p][i - a_off].x : e == 1 ? a[p][i - a_off].y : e == 2 ? a[p][i - a_off].z : a[p][i - a_off].w;
#pragma unroll
                    for (int j = 0; j < CT; ++j) {
                        const float bv = e == 0 ? b[j].x : e == 1 ? b[j].y : e == 2 ? b[j].z : b[j].w;
                        acc[p * CT + j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[p * CT + j], 0, 0, 0);
                    }
                }
        }
    };
    auto mma_all = [&](f32x16 (&acc)[PT * CT], const float4 (&a)[PT][NQ]) { mma(acc, a, IC<0>{}, IC<NQ>{}, IC<0>{}); };
    // epilogue straight from the accumulators: register q of tile (p, j) = pixel row(q, hh) of pixel tile p, cout co + j
    auto put = [&](float *dst, const f32x16 (&acc)[PT * CT], int p, const float4 (&rs)[RES ? 16 : 1], int q) {
        float v[CT];
#pragma unroll
        for (int e = 0; e < CT; ++e) v[e] = acc[p * CT + e][q];
        if constexpr (!GEMM) {
#pragma unroll
            for (int e = 0; e < CT; ++e) v[e] = __fadd_rn(__fmul_rn(v[e], sc[e]), sh[e]);
        }
        if constexpr (RES) {
            v[0] = __fadd_rn(v[0], rs[q].x); v[1] = __fadd_rn(v[1], rs[q].y);
            v[2] = __fadd_rn(v[2], rs[q].z); v[3] = __fadd_rn(v[3], rs[q].w);
        }
        if constexpr (RELU) {
#pragma unroll
            for (int e = 0; e < CT; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        if constexpr (CT == 4) *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        else *reinterpret_cast<float2 *>(dst) = make_float2(v[0], v[1]);
    };
    auto epi_part = [&](const f32x16 (&acc)[PT * CT], const float4 (&rs)[RES ? 16 : 1], int64_t t, auto q0_c, auto q1_c) {    // full tiles, rows [q0, q1)
#pragma unroll
        for (int p = 0; p < PT; ++p) {
            float *op = MODE != 0 ? ob + (t * ROWS + PW_ROWS * p) * ops : ob + (t * ROWS + PW_ROWS * p + 4 * hh) * ops + co;
#pragma unroll
            for (int q = decltype(q0_c)::value; q < decltype(q1_c)::value; ++q)
                put(op + (int64_t)((q & 3) + 8 * (q >> 2)) * ops + (MODE != 0 ? o_lane : 0u), acc, p, rs, q);
        }
    };
    auto epi = [&](const f32x16 (&acc)[PT * CT], const float4 (&rs)[RES ? 16 : 1], int64_t t) { epi_part(acc, rs, t, IC<0>{}, IC<16>{}); };

    // the tiles t_first, t_first + stride_t, ... below t_end (<= n_tiles) of the current entry
    auto run = [&](const int64_t t_first, const int64_t stride_t, const int64_t t_end) {
        // ---- full tiles, software-pipelined over two register sets: in phase i the residual of tile i and the
        // activations of tile i + 1 are requested, then the MFMAs of tile i (into acc[i % 2]) and the epilogue of tile
        // i - 1 (out of acc[(i - 1) % 2]) sit in ONE basic block, so that the scheduler can slot the epilogue's vector ALU
        // work and stores between the matrix instructions -- with one wave per SIMD nothing else would fill the matrix
        // pipe's shadow.  Loads are consumed one phase (64-512 MFMAs, 2-14 us) after they were issued.
        const int64_t f_end = n_full < t_end ? n_full : t_end;
        if (t_first < f_end) {
            const int64_t m = (f_end - t_first + stride_t - 1) / stride_t;        // tiles of this wave
            auto tile = [&](int64_t i) { return t_first + (i < m ? i : m - 1) * stride_t; };   // (past the end: re-request the last)
            if constexpr (MODE == 0) {
                float4 a0[PT][NQ], a1[PT][NQ], rs0[RES ? 16 : 1], rs1[RES ? 16 : 1];
                f32x16 acc0[PT * CT], acc1[PT * CT];
                load_a(tile(0), a0, xb);
                load_rs(tile(0), rs0);
                load_a(tile(1), a1, xb);
                mma_all(acc0, a0);
                int64_t i = 1;
                for (; i + 1 < m; i += 2) {
                    load_rs(tile(i), rs1);
                    load_a(tile(i + 1), a0, xb);
                    mma_all(acc1, a1);
                    epi(acc0, rs0, tile(i - 1));
                    load_rs(tile(i + 1), rs0);
                    load_a(tile(i + 2), a1, xb);
                    mma_all(acc0, a0);
                    epi(acc1, rs1, tile(i));
                }
                if (i < m) {                               // one more tile (odd index), then its epilogue
                    load_rs(tile(i), rs1);
                    mma_all(acc1, a1);
                    epi(acc0, rs0, tile(i - 1));
                    epi(acc1, rs1, tile(i));
                } else {
                    epi(acc0, rs0, tile(i - 1));
                }
            } else if constexpr (MODE == 1) {
                // Cin = 256.  The matrix instructions take their A / B operands from the 256 architectural registers only
                // (the accumulators sit in the other 256), and so does the epilogue's vector ALU work, for which the
                // compiler copies the finished tile's accumulators over (64): two whole activation sets (2 x 128) or even
                // one next to the residual (64) do not fit.  So a phase (tile i: 512 MFMAs, ~13 us) is eight fenced eighths of
                // 64 MFMAs, one 32-channel slab each, and the activations go through a RING OF FOUR SLABS (64 registers):
                // as soon as eighth e has consumed slab e, slab e + 4 -- of tile i + 1 from e = 4 on -- is requested into
                // the registers it has just freed, three eighths (5 us) before its use.  ONE residual set: the residual of
                // tile i - 1 is requested at the start of phase i and consumed by the epilogue of tile i - 1, which runs in
                // the shadow of eighths 4-7 (four output rows each), half a phase (6 us) later.  The fences keep the scheduler
                // from undoing this order (hoisting a phase's LDS reads or requests in front of the MFMAs that free their
                // registers, or the epilogue in front of its residual's latency).
                constexpr int NE = NQ / 8;
                float4 a[PT][4 * NE], rs[16];
                f32x16 acc0[PT * CT], acc1[PT * CT];
                auto load_k = [&](int64_t t, auto slab_c) {         // slab (NE pieces) of tile t into its slot, slab % 4
                    constexpr int off = decltype(slab_c)::value * NE, slot = (decltype(slab_c)::value & 3) * NE;
#pragma unroll
                    for (int p = 0; p < PT; ++p) {
                        const float *ap = xb + (t * ROWS + PW_ROWS * p) * CIN + a_lane;
#pragma unroll
                        for (int k = 0; k < NE; ++k) a[p][slot + k] = *reinterpret_cast<const float4 *>(ap + S * ((off + k) / QS) + 4 * ((off + k) % QS));
                    }
                };
                // tile t_n into acc_n; epilogue of tile t_o out of acc_o; the first four slabs of tile t_x requested
                auto phase = [&](f32x16 (&acc_n)[PT * CT], int64_t t_n, const f32x16 (&acc_o)[PT * CT], int64_t t_o, auto with_epi, int64_t t_x, auto with_next) {
                    if constexpr (decltype(with_epi)::value) load_rs(t_o, rs);
                    auto eighth = [&](auto e_c) {
                        constexpr int E = decltype(e_c)::value;
                        mma(acc_n, a, IC<NE * E>{}, IC<NE * E + NE>{}, IC<NE * (E & 4)>{});
                        if constexpr (decltype(with_epi)::value && E >= 4) epi_part(acc_o, rs, t_o, IC<4 * (E - 4)>{}, IC<4 * (E - 4) + 4>{});
                        __builtin_amdgcn_sched_barrier(0);
                        if constexpr (E < 4) load_k(t_n, IC<E + 4>{});
                        else if constexpr (decltype(with_next)::value) load_k(t_x, IC<E - 4>{});
                    };
                    eighth(IC<0>{}); eighth(IC<1>{}); eighth(IC<2>{}); eighth(IC<3>{});
                    eighth(IC<4>{}); eighth(IC<5>{}); eighth(IC<6>{}); eighth(IC<7>{});
                };
                load_k(tile(0), IC<0>{}); load_k(tile(0), IC<1>{}); load_k(tile(0), IC<2>{}); load_k(tile(0), IC<3>{});
                phase(acc0, tile(0), acc1, 0, IC<0>{}, tile(1), IC<1>{});
                int64_t i = 1;
                for (; i + 1 < m; i += 2) {
                    phase(acc1, tile(i), acc0, tile(i - 1), IC<1>{}, tile(i + 1), IC<1>{});
                    phase(acc0, tile(i + 1), acc1, tile(i), IC<1>{}, tile(i + 2), IC<1>{});
                }
                if (i < m) {                               // one more tile (odd index), then its epilogue
                    phase(acc1, tile(i), acc0, tile(i - 1), IC<1>{}, 0, IC<0>{});
                    load_rs(tile(i), rs);
                    epi(acc1, rs, tile(i));
                } else {
                    load_rs(tile(i - 1), rs);
                    epi(acc0, rs, tile(i - 1));
                }
            }
        }
        // ---- the entry's one partial tile (M % ROWS rows), by the wave whose turn it would be: clamped loads, masked stores
        if (n_full < t_end && n_full >= t_first && (n_full - t_first) % stride_t == 0) {
            const int64_t p0 = n_full * ROWS;
            float4 a[PT][NQ], rs[RES ? 16 : 1];
            f32x16 acc[PT * CT];
#pragma unroll
            for (int p = 0; p < PT; ++p) {
                const int64_t pr = p0 + PW_ROWS * p + r;
                const float *ap = xb + (pr < g.M ? pr : g.M - 1) * CIN + hh * (S / 2);
#pragma unroll
                for (int i = 0; i < NQ; ++i) a[p][i] = *reinterpret_cast<const float4 *>(ap + S * (i / QS) + 4 * (i % QS));
            }
            if constexpr (RES) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    int64_t p = p0 + (q & 3) + 8 * (q >> 2) + 4 * hh;
                    p = p < g.M ? p : g.M - 1;
                    rs[q] = *reinterpret_cast<const float4 *>(g.res + p * g.res_ps + co);
                }
            }
            mma_all(acc, a);
#pragma unroll
            for (int p = 0; p < PT; ++p)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int64_t px = p0 + PW_ROWS * p + (q & 3) + 8 * (q >> 2) + 4 * hh;
                    if (px < g.M) put(ob + px * ops + co, acc, p, rs, q);
                }
        }
    };

    if constexpr (GEMM) {
        // block k of n takes the tiles [G k / n, G (k + 1) / n) of the launch's G = batch x n_tiles (entry, tile) sequence,
        // its four waves alternating inside the part that lies in one entry
        const int64_t G = (int64_t)g.batch * n_tiles;
        int64_t lo = G * bid / gridDim.x;
        const int64_t hi = G * (bid + 1) / gridDim.x;
        while (lo < hi) {
            const int64_t b = lo / n_tiles, t0 = lo - b * n_tiles;
            const int64_t t1 = hi - lo < n_tiles - t0 ? t0 + (hi - lo) : n_tiles;
            xb = g.x + b * g.x_bs;
            wb = g.w + b * g.w_bs;
            ob = g.out + b * g.out_bs;
            stage();
            run(t0 + wave, PW_THREADS / 64, t1);
            __syncthreads();                           // every wave is done with this entry's weights
            lo += t1 - t0;
        }
    } else {
        stage();
        run((int64_t)pb * (PW_THREADS / 64) + wave, (int64_t)g.pix_blocks * (PW_THREADS / 64), n_tiles);
    }
}

static bool pw_off()
{
    static const char *off = getenv("EMP_CONV_NO_WS");         // experiments only (A/B against the tiled kernel)
    return off && off[0] == '1';
}

static bool pw_off3()
{
    static const char *off = getenv("EMP_CONV_NO_WS3");        // experiments only: kind 3 off (its shapes back on the tiled kernel)
    return pw_off() || (off && off[0] == '1');
}

// Shapes the weight-stationary kernel takes (everything else stays on conv_igemm_f32_kernel): 1x1, stride 1, no padding,
// and enough pixels to give every CU's waves several tiles.
//   1: Cin 64 or 128, whole 128-cout groups (conv3 + identity, the shortcut projection): K-slab 64;
//   2: 256 -> 64, 64 -> 64, 256 -> 128 (the bottleneck's conv1 in layer1 / layer2): the K-slab of the tiled kernel's plan,
//      which the caller passes to the launcher; without a residual only (emp_conv_bn_act_nhwc also checks that the
//      plan's slab is 16 -- it always is at these sizes unless an experiment switch forces 32).
//   3: Cin 256, whole 128-cout groups, WITH a residual (layer3's conv3 + identity): K-slab 32, the order of the tiled
//      kernel's residual-prefetch plan (emp_conv_bn_act_nhwc takes it only when a residual is present and that plan says
//      so), so emp_conv_k_slab_geom keeps its answer for these shapes.  Its tile is 512 MFMAs long and its pipeline two
//      tiles deep, so it wants sixteen tiles per wave: pixels x cout groups >= 8 x 65 536 (256 -> 128 + residual on 65 536
//      pixels, two tiles per wave, measured 0.052 ms against the tiled kernel's 0.049: profiles/ws_conv3_k256.md).
// (the launcher additionally wants scale AND shift -- every call site on the path is conv + BatchNorm)
extern "C" __attribute__((visibility("hidden"))) int emp_conv1x1_ws_kind(int64_t M, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu,
                                                                         int has_residual)
{
    if (pw_off()) return 0;
    if (!(KH == 1 && KW == 1 && stride == 1 && pad == 0 && relu != 2)) return 0;
    if ((Cin == 64 || Cin == 128) && Cout % 128 == 0 && Cout / 128 <= 8 && M >= PW_MIN_ROWS) return 1;
    if (!has_residual && M >= PW_MIN_ROWS_PLAN && ((Cin == 256 && Cout == 64) || (Cin == 64 && Cout == 64) || (Cin == 256 && Cout == 128)))
        return 2;
    if (has_residual && Cin == 256 && Cout % 128 == 0 && Cout / 128 <= 8 && M >= PW_MIN_ROWS && M * (Cout / 128) >= 8 * PW_MIN_ROWS &&
        !pw_off3())
        return 3;
    return 0;
}

extern "C" int emp_conv1x1_ws_eligible(int64_t M, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu)
{
    return emp_conv1x1_ws_kind(M, Cin, Cout, KH, KW, stride, pad, relu, 0) != 0;    // (with a residual: emp_conv1x1_ws_kind_for)
}

// the batched GEMM emp_gemm_nt_batched hands over: K and N 64 or 128, the plan's K-slab 16, batch x M rows enough
extern "C" __attribute__((visibility("hidden"))) int emp_gemm_ws_eligible(int batch, int64_t M, int N, int K, int slab)
{
    if (pw_off()) return 0;
    return (K == 64 || K == 128) && (N == 64 || N == 128) && slab == 16 && M >= PW_ROWS && (int64_t)batch * M >= PW_MIN_ROWS_PLAN;
}

template <int KS, int S, int CT, int PT, bool GEMM, bool RES, int MODE = 0>
static void pw_go(const PwGeom &g, int blocks, hipStream_t st)
{
    if (g.relu) {
        if constexpr (!GEMM) hipLaunchKernelGGL((conv1x1_ws_kernel<KS, S, CT, PT, GEMM, RES, true, MODE>), dim3(blocks), dim3(PW_THREADS), 0, st, g);
    } else {
        hipLaunchKernelGGL((conv1x1_ws_kernel<KS, S, CT, PT, GEMM, RES, false, MODE>), dim3(blocks), dim3(PW_THREADS), 0, st, g);
    }
}

// one block per CU (256 CUs): pix_blocks x groups blocks, pix_blocks a multiple of 8 (XCDs)
static int pw_grid(PwGeom &g, int groups)
{
    g.groups = groups;
    int pix = 256 / groups;
    pix = pix / 8 * 8;
    if (pix < 8) pix = 8;
    g.pix_blocks = pix;
    return pix * groups;
}

// launches so far, by kind (emp_conv1x1_ws_launches): lets a test see WHICH kernel a call of emp_conv_bn_act_nhwc took --
// the dispatch also looks at alignment, pixel strides and the tiled plan, which the kind queries do not know
static std::atomic<int64_t> pw_launches[4];

extern "C" int64_t emp_conv1x1_ws_launches(int kind)
{
    return kind >= 1 && kind <= 3 ? pw_launches[kind].load() : -1;
}

// called by emp_conv_bn_act_nhwc for eligible shapes (pointers and strides already checked for 16-byte alignment);
// kind as emp_conv1x1_ws_kind answered (2: no residual, K-slab 16; 3: residual present, K-slab 32)
extern "C" __attribute__((visibility("hidden"))) int emp_conv1x1_ws_launch(int kind, const float *x, const float *w, const float *scale, const float *shift,
                                     const float *res, int64_t res_ps, int relu, int64_t M, int Cin, int Cout,
                                     float *out, int64_t out_ps, void *stream)
{
    PwGeom g;
    g.x = x; g.w = w; g.scale = scale; g.shift = shift; g.res = res; g.out = out;
    g.M = M; g.out_ps = out_ps; g.res_ps = res_ps; g.Cin = Cin; g.Cout = Cout; g.relu = relu;
    g.batch = 1; g.x_bs = g.w_bs = g.out_bs = 0;
    const int blocks = pw_grid(g, kind == 2 ? 1 : Cout / 128);
    hipStream_t st = emp_stream(stream);
    if (kind == 3) {
        pw_go<4, 32, 4, 1, false, true, 1>(g, blocks, st);                        // 256 -> 128 n + residual
    } else if (kind == 1) {
        if (Cin == 64) { if (res) pw_go<1, 64, 4, 1, false, true>(g, blocks, st); else pw_go<1, 64, 4, 1, false, false>(g, blocks, st); }
        else { if (res) pw_go<2, 64, 4, 1, false, true>(g, blocks, st); else pw_go<2, 64, 4, 1, false, false>(g, blocks, st); }
    } else {
        if (Cin == 64) pw_go<1, 16, 2, 2, false, false>(g, blocks, st);           // 64 -> 64
        else if (Cout == 64) pw_go<4, 16, 2, 1, false, false>(g, blocks, st);     // 256 -> 64
        else pw_go<4, 16, 4, 1, false, false>(g, blocks, st);                     // 256 -> 128
    }
    EMP_CHECK_LAUNCH("emp_conv_bn_act_nhwc(1x1 weight-stationary)");
    pw_launches[kind]++;
    return EMP_OK;
}

// called by emp_gemm_nt_batched for eligible shapes (A, B, C 16-byte aligned)
extern "C" __attribute__((visibility("hidden"))) int emp_gemm_ws_launch(const float *A, const float *B, int batch, int64_t M, int N, int K, float *C,
                                                                        void *stream)
{
    PwGeom g;
    g.x = A; g.w = B; g.scale = g.shift = g.res = nullptr; g.out = C;
    g.M = M; g.out_ps = N; g.res_ps = N; g.Cin = K; g.Cout = N; g.relu = 0;
    g.batch = batch; g.x_bs = M * K; g.w_bs = (int64_t)N * K; g.out_bs = M * N;
    g.groups = 1; g.pix_blocks = 256;
    hipStream_t st = emp_stream(stream);
    if (K == 64) { if (N == 64) pw_go<1, 16, 2, 2, true, false>(g, 256, st); else pw_go<1, 16, 4, 1, true, false>(g, 256, st); }
    else { if (N == 64) pw_go<2, 16, 2, 2, true, false>(g, 256, st); else pw_go<2, 16, 4, 1, true, false>(g, 256, st); }
    EMP_CHECK_LAUNCH("emp_gemm_nt_batched(weight-stationary)");
    return EMP_OK;
}

// the kind emp_conv_bn_act_nhwc takes for a geometry with / without a residual (0: the tiled kernel), given aligned operands
extern "C" int emp_conv1x1_ws_kind_for(int64_t M, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu, int has_residual)
{
    return emp_conv1x1_ws_kind(M, Cin, Cout, KH, KW, stride, pad, relu, has_residual);
}
