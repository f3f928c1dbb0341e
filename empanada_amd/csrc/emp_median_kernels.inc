// The recursive median + harden kernels, written ONCE and compiled once per slice -> pointer selection: emp_pixel.hip
// includes this file twice, with the MEDIAN_* macros set to the whole stack in one tensor (emp_median_harden_stack: the
// macros expand to the plain indexing these kernels were written with, so their code is what it was) and to the virtual
// stack hist | prob | halo of emp_median_harden_window (WindowSel).  The filter never names a tensor:
//   MEDIAN_KERNEL(form)           the kernel's name
//   MEDIAN_SRC_PARAM              first parameter: where the raw slices are
//   MEDIAN_OUT_PROB_PARAM         the out_prob parameter (no __restrict__ where it may be the history)
//   MEDIAN_LANE(src, p, C)        declares the source of pixel p's lane
//   MEDIAN_LD(src, z, idx)        raw value at element idx = (z * C + c) * HW of that source; z says which tensor
//   MEDIAN_IF_SEM(s) / MEDIAN_IF_PROB(s)      guard of the two stores of slice s
//   MEDIAN_SEM_ROW(s) / MEDIAN_PROB_ROW(s)    the output row slice s is stored at
// Every selection is uniform per slice: the window form adds scalar compares, no divergence.  The macros are undefined
// at the end of this file.

// ------------------------------------------------------------------------------------------
// P1+P2, C == 1: one thread per pixel walks the stack in z with the filter window in registers.
// Loads of the next PF slices are issued before the current PF medians are computed so that
// every lane keeps PF dword loads in flight (the recursion itself is serial in z).
// Algorithmic traffic: 4 B read + 1 B write per voxel (+4 B if out_prob).
template <int KS>
__global__ __launch_bounds__(256) void MEDIAN_KERNEL(c1)(MEDIAN_SRC_PARAM, int D,
                                                               int64_t HW, float thr,
                                                               uint8_t *__restrict__ out_sem,
                                                               MEDIAN_OUT_PROB_PARAM)
{
    constexpr int M = KS / 2;
    constexpr int PF = 8;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < HW;
         p += (int64_t)gridDim.x * blockDim.x) {
        MEDIAN_LANE(src, p, 1);
        float win[KS];
        // slices 0..KS-2 enter the window; the first M of them pass through raw
#pragma unroll
        for (int i = 0; i < KS - 1; ++i) win[i] = MEDIAN_LD(src, i, (int64_t)i * HW);
#pragma unroll
        for (int i = 0; i < M; ++i) {
            MEDIAN_IF_SEM(i) out_sem[(int64_t)MEDIAN_SEM_ROW(i) * HW + p] = win[i] >= thr ? 1 : 0;
            MEDIAN_IF_PROB(i) out_prob[(int64_t)MEDIAN_PROB_ROW(i) * HW + p] = win[i];
        }
        float cur[PF], nxt[PF];
        const int s_end = D - M;  // filtered slices are [M, s_end)
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            int z = M + u + M;
            cur[u] = (z < D) ? MEDIAN_LD(src, z, (int64_t)z * HW) : 0.f;
        }
        for (int s0 = M; s0 < s_end; s0 += PF) {
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                int z = s0 + PF + u + M;
                nxt[u] = (z < D) ? MEDIAN_LD(src, z, (int64_t)z * HW) : 0.f;
            }
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                int s = s0 + u;
                if (s < s_end) {
                    win[KS - 1] = cur[u];
                    float med = median_regs<KS>(win);
                    MEDIAN_IF_SEM(s) out_sem[(int64_t)MEDIAN_SEM_ROW(s) * HW + p] = med >= thr ? 1 : 0;
                    MEDIAN_IF_PROB(s) out_prob[(int64_t)MEDIAN_PROB_ROW(s) * HW + p] = med;
                    // slide: the filtered value replaces the raw one (recursive filter)
                    win[M] = med;
#pragma unroll
                    for (int i = 0; i < KS - 1; ++i) win[i] = win[i + 1];
                }
            }
#pragma unroll
            for (int u = 0; u < PF; ++u) cur[u] = nxt[u];
        }
        // tail: win[M .. KS-2] hold the raw slices D-M .. D-1
#pragma unroll
        for (int i = 0; i < M; ++i) {
            int s = D - M + i;
            float v = win[M + i];
            MEDIAN_IF_SEM(s) out_sem[(int64_t)MEDIAN_SEM_ROW(s) * HW + p] = v >= thr ? 1 : 0;
            MEDIAN_IF_PROB(s) out_prob[(int64_t)MEDIAN_PROB_ROW(s) * HW + p] = v;
        }
    }
}

// P1+P2, C > 1: same scan, one filter window per channel kept in LDS ([c][k][tid] -> conflict
// free), argmax over the filtered channels (first maximum wins, like torch.argmax).
template <int KS>
__global__ __launch_bounds__(256) void MEDIAN_KERNEL(mc)(MEDIAN_SRC_PARAM, int D,
                                                               int C, int64_t HW,
                                                               uint8_t *__restrict__ out_sem,
                                                               MEDIAN_OUT_PROB_PARAM)
{
    extern __shared__ float lds[];  // C * KS * blockDim.x
    constexpr int M = KS / 2;
    const int tid = threadIdx.x;
    const int nt = blockDim.x;
    for (int64_t p0 = (int64_t)blockIdx.x * nt; p0 < HW; p0 += (int64_t)gridDim.x * nt) {
        int64_t p = p0 + tid;
        bool live = p < HW;
        if (live) {
            MEDIAN_LANE(src, p, C);
            for (int c = 0; c < C; ++c)
                for (int i = 0; i < KS - 1; ++i)
                    lds[(c * KS + i) * nt + tid] = MEDIAN_LD(src, i, ((int64_t)i * C + c) * HW);
            for (int s = 0; s < D; ++s) {
                bool filt = (s >= M) && (s < D - M);
                float best = -INFINITY;
                int arg = 0;
                for (int c = 0; c < C; ++c) {
                    float v;
                    if (filt) {
                        float w[KS];
                        // slot of slice z is z % KS; the incoming slice s+M overwrites s-M-1
                        lds[(c * KS + (s + M) % KS) * nt + tid] = MEDIAN_LD(src, s + M, ((int64_t)(s + M) * C + c) * HW);
#pragma unroll
                        for (int i = 0; i < KS; ++i) w[i] = lds[(c * KS + i) * nt + tid];
                        v = median_regs<KS>(w);
                        lds[(c * KS + s % KS) * nt + tid] = v;
                    } else {
                        v = (KS == 1) ? MEDIAN_LD(src, s, ((int64_t)s * C + c) * HW)
                                      : lds[(c * KS + s % KS) * nt + tid];
                    }
                    MEDIAN_IF_PROB(s) out_prob[((int64_t)MEDIAN_PROB_ROW(s) * C + c) * HW + p] = v;
                    if (v > best) { best = v; arg = c; }
                }
                MEDIAN_IF_SEM(s) out_sem[(int64_t)MEDIAN_SEM_ROW(s) * HW + p] = (uint8_t)arg;
            }
        }
        __syncthreads();
    }
}

// The same for C <= MC_CMAX channels with the incoming slices PREFETCHED: the loads of the next MC_PF slices (all
// channels: MC_PF x C dword loads per lane) are in flight while the current slice is filtered -- the form above issues
// every load right before its use and ran at 0.6 TB/s on C = 5 (one HBM latency per slice and channel, 16 waves per CU).
// Filtered steps t = 0 .. D - 2M - 1 (slice s = M + t, incoming slice s + M) are unrolled by MC_PF so that the prefetch
// registers are indexed statically.
template <int KS>
__global__ __launch_bounds__(256) void MEDIAN_KERNEL(mc8)(MEDIAN_SRC_PARAM, int D, int C,
                                                                int64_t HW, uint8_t *__restrict__ out_sem,
                                                                MEDIAN_OUT_PROB_PARAM)
{
    extern __shared__ float lds[];  // C * KS * blockDim.x, [c][slot][tid]; a lane only touches its own column
    constexpr int M = KS / 2;
    const int tid = threadIdx.x;
    const int nt = blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * nt + tid; p < HW; p += (int64_t)gridDim.x * nt) {
        MEDIAN_LANE(src, p, C);
        const int64_t cs = HW;                                    // channel stride; slice stride = C * HW
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int i = 0; i < KS - 1; ++i) lds[(c * KS + i) * nt + tid] = MEDIAN_LD(src, i, ((int64_t)i * C + c) * cs);
        float nx[MC_PF][MC_CMAX];
#pragma unroll
        for (int j = 0; j < MC_PF; ++j)
#pragma unroll
            for (int c = 0; c < MC_CMAX; ++c)
                nx[j][c] = (c < C && KS - 1 + j < D) ? MEDIAN_LD(src, KS - 1 + j, ((int64_t)(KS - 1 + j) * C + c) * cs) : 0.f;
        // the first M slices pass through raw
        for (int s = 0; s < M; ++s) {
            float best = -INFINITY;
            int arg = 0;
            for (int c = 0; c < C; ++c) {
                const float v = lds[(c * KS + s) * nt + tid];
                MEDIAN_IF_PROB(s) out_prob[((int64_t)MEDIAN_PROB_ROW(s) * C + c) * cs + p] = v;
                if (v > best) { best = v; arg = c; }
            }
            MEDIAN_IF_SEM(s) out_sem[(int64_t)MEDIAN_SEM_ROW(s) * HW + p] = (uint8_t)arg;
        }
        const int n_f = D - 2 * M;                                // filtered slices (D >= KS: at least one)
        int slot_in = (KS - 1) % KS, slot_s = M % KS;             // ring slots of the incoming slice and of slice s
        for (int t0 = 0; t0 < n_f; t0 += MC_PF) {
#pragma unroll
            for (int j = 0; j < MC_PF; ++j) {
                const int t = t0 + j;
                if (t < n_f) {                                     // block-uniform
                    const int s = M + t, zin = s + M;
                    float best = -INFINITY;
                    int arg = 0;
#pragma unroll
                    for (int c = 0; c < MC_CMAX; ++c) {
                        if (c < C) {
                            float w[KS];
                            lds[(c * KS + slot_in) * nt + tid] = nx[j][c];
                            nx[j][c] = (zin + MC_PF < D) ? MEDIAN_LD(src, zin + MC_PF, ((int64_t)(zin + MC_PF) * C + c) * cs) : 0.f;
#pragma unroll
                            for (int i = 0; i < KS; ++i) w[i] = lds[(c * KS + i) * nt + tid];
                            const float v = median_regs<KS>(w);
                            lds[(c * KS + slot_s) * nt + tid] = v;        // recursive: later windows see the filtered value
                            MEDIAN_IF_PROB(s) out_prob[((int64_t)MEDIAN_PROB_ROW(s) * C + c) * cs + p] = v;
                            if (v > best) { best = v; arg = c; }
                        }
                    }
                    MEDIAN_IF_SEM(s) out_sem[(int64_t)MEDIAN_SEM_ROW(s) * HW + p] = (uint8_t)arg;
                    slot_in = slot_in + 1 == KS ? 0 : slot_in + 1;
                    slot_s = slot_s + 1 == KS ? 0 : slot_s + 1;
                }
            }
        }
        // the last M slices pass through raw
        for (int s = D - M; s < D; ++s) {
            float best = -INFINITY;
            int arg = 0;
            for (int c = 0; c < C; ++c) {
                const float v = lds[(c * KS + s % KS) * nt + tid];
                MEDIAN_IF_PROB(s) out_prob[((int64_t)MEDIAN_PROB_ROW(s) * C + c) * cs + p] = v;
                if (v > best) { best = v; arg = c; }
            }
            MEDIAN_IF_SEM(s) out_sem[(int64_t)MEDIAN_SEM_ROW(s) * HW + p] = (uint8_t)arg;
        }
    }
}

#undef MEDIAN_KERNEL
#undef MEDIAN_SRC_PARAM
#undef MEDIAN_OUT_PROB_PARAM
#undef MEDIAN_LANE
#undef MEDIAN_LD
#undef MEDIAN_IF_SEM
#undef MEDIAN_IF_PROB
#undef MEDIAN_SEM_ROW
#undef MEDIAN_PROB_ROW
