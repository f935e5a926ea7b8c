// ctc.hip — the CTC head's device path: gathered log-softmax + argmax, batched sequence likelihood, greedy decode.
//
// Replaces (reference, paths relative to the HubertFA repository):
//   * F.log_softmax(ctc_logits) + nn.CTCLoss(reduction="none")   networks/task/forced_alignment.py:256-272,
//                                                                networks/loss/GHMLoss.py:12-56  -> hfa_ctc_prologue,
//                                                                                                   hfa_ctc_forward
//   * AlignmentDecoder.ctc (argmax + collapse)                   tools/alignment_decoder.py:145-150 -> hfa_ctc_prologue,
//                                                                                                   hfa_ctc_greedy
//
// Forward (one workgroup per utterance, the parallel shape of viterbi.hip's DP in the log-sum-exp semiring): the
// 2L + 1 extended states are held as L + 1 (blank_j, label_j) pairs, state 2j and 2j + 1; pair L's label does not
// exist.  With b = blank, l = label, e = this frame's gathered emissions:
//     b_j' = e[0]     + lse(b_j, l_{j-1})
//     l_j' = e[j + 1] + lse(l_j, b_j, l_{j-1} if target j != target j-1)
// so the only value that crosses lanes per step is the label of the pair below (one DPP move; an LDS slot across
// waves).  Each lane owns P contiguous pairs; emission rows are prefetched a group of steps ahead with unconditional,
// clamped loads (see viterbi.hip on why loads in divergent branches defeat the prefetch).
//
// Numerics: alpha is f32 and REBASED: after every step t with t % 16 == 15 the row maximum is subtracted from every
// state and added to a per-utterance f64 offset, so alpha stays within a few hundred of zero whatever T is and its
// ulp does not grow with t.  nll = -(offset + lse(b_L, l_{L-1})) in f64.  Unreachable states are -inf; a log-sum-exp
// whose maximum is -inf subtracts 0 instead, so -inf - (-inf) never reaches an exp, without a branch.  The per-state
// arithmetic does not depend on P or on the number of waves (max is exact), so an utterance gives the same bits alone
// and inside any batch.  Built with -ffp-contract=off for the same reason.
#include "hfa_common.h"

namespace {

using hfa::neg_inf;

constexpr int kMaxV = 1024;             // as hfa_lattice_prologue
constexpr int kMaxLabels = 8191;        // 8192 pairs: 16 waves x 64 lanes x 8 pairs
constexpr int kRebase = 16;             // steps between rebases (a power of two)
constexpr int kProThreads = 256;

__device__ __forceinline__ float from_lane_below(float v) {   // DPP wave_shr:1, lane 0 receives -inf
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(neg_inf()), __float_as_int(v), 0x138, 0xF, 0xF,
                                                      false));
}

// log(exp(a) + exp(b)); -inf when both are
__device__ __forceinline__ float lse2(float a, float b) {
    const float hi = fmaxf(a, b), lo = fminf(a, b);
    const float mm = hi == neg_inf() ? 0.0f : hi;
    return hi + logf(1.0f + expf(lo - mm));
}
// log(exp(a) + exp(b) + exp(c)); -inf when all are
__device__ __forceinline__ float lse3(float a, float b, float c) {
    const float hi = fmaxf(fmaxf(a, b), c), lo = fminf(fminf(a, b), c);
    const float mid = __builtin_amdgcn_fmed3f(a, b, c);
    const float mm = hi == neg_inf() ? 0.0f : hi;
    return hi + logf(1.0f + expf(mid - mm) + expf(lo - mm));
}

// ---- prologue: one wave per frame row ---------------------------------------------------------------------------
__global__ __launch_bounds__(kProThreads) void ctc_prologue_kernel(
    int Tmax, int V, int Lmax, const int32_t* __restrict__ Tv, const int32_t* __restrict__ Lv,
    const float* __restrict__ logits, long long ld, long long bs, int blank_col, int label_off,
    const int32_t* __restrict__ targets, float* __restrict__ emis, int32_t* __restrict__ best) {
    __shared__ float xs[kProThreads / 64][kMaxV];
    const int b = blockIdx.y;
    const int T = min(Tv[b], Tmax);
    const int L = min(Lv[b], Lmax);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* xw = xs[w];
    const int32_t* tg = targets + (size_t)b * Lmax;
    const int tstride = gridDim.x * (kProThreads / 64);
    for (int t = blockIdx.x * (kProThreads / 64) + w; t < T; t += tstride) {   // rows t >= T[b] are never read
        const float* xr = logits + b * bs + t * ld;
        float m = neg_inf();
        int am = 0x7fffffff;
        for (int c = lane; c < V; c += 64) {
            const float x = xr[c == 0 ? blank_col : c + label_off];
            xw[c] = x;
            if (x > m || am == 0x7fffffff) {     // ascending c: the lowest class of this lane's maximum
                m = x;
                am = c;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {       // (max, lowest class) over the wave: np.argmax's first index on ties
            const float mo = __shfl_xor(m, o, 64);
            const int ao = __shfl_xor(am, o, 64);
            if (mo > m || (mo == m && ao < am) || am == 0x7fffffff) {
                m = mo;
                am = ao;
            }
        }
        float sum = 0.0f;
        for (int c = lane; c < V; c += 64) sum += expf(xw[c] - m);
        sum = hfa::wave_sum(sum);
        const float lse = logf(sum);
        __builtin_amdgcn_wave_barrier();
        float* er = emis + ((size_t)b * Tmax + t) * (Lmax + 1);
        for (int j = lane; j <= L; j += 64) {    // column 0 the blank, column j target j - 1
            const int c = j == 0 ? 0 : tg[j - 1];
            er[j] = (xw[c] - m) - lse;
        }
        if (lane == 0) best[(size_t)b * Tmax + t] = am;
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- forward ----------------------------------------------------------------------------------------------------
// P pairs per lane, NW waves, G steps per prefetch group, two groups in flight (2 G P emission registers per lane).
template <int P, int NW, int G>
__global__ __launch_bounds__(64 * NW) void ctc_forward_kernel(
    int Tmax, int Lmax, const int32_t* __restrict__ Tv, const int32_t* __restrict__ Lv,
    const float* __restrict__ emis, const int32_t* __restrict__ targets, double* __restrict__ nll) {
    static_assert(G <= 64 && kRebase % G == 0, "a group's blank emissions fit one wave's lanes");
    constexpr int R = 2;
    __shared__ float xl[2][NW];          // a wave's last label, for lane 0 of the next wave (double-buffered)
    __shared__ float red[2][NW];         // rebase: the waves' maxima
    __shared__ float fin[2];             // b_L, l_{L-1} after the last step
    const int b = blockIdx.x;
    const int g = threadIdx.x;
    const int lane = g & 63, wave = g >> 6;
    const int T = min(Tv[b], Tmax);
    const int L = min(Lv[b], Lmax);
    const int pitch = Lmax + 1;
    const float* em = emis + (size_t)b * Tmax * pitch;
    const int32_t* tg = targets + (size_t)b * Lmax;
    if (g < 2) fin[g] = neg_inf();

    const int j0 = g * P;
    float bl[P], lb[P];                  // alpha of the blank / label state of this lane's pairs
    bool lvalid[P], allow[P];
    int col[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int j = j0 + i;
        lvalid[i] = j < L;
        col[i] = lvalid[i] ? j + 1 : 0;                       // clamped: a lane past L loads the blank column
        const int cur = lvalid[i] ? tg[j] : 0;
        const int prev = (lvalid[i] && j >= 1) ? tg[j - 1] : 0;
        allow[i] = lvalid[i] && j >= 1 && cur != prev;
        bl[i] = j == 0 ? 0.0f : neg_inf();                    // the virtual row before frame 0: all mass on state 0
        lb[i] = neg_inf();
    }
    double offset = 0.0;

    float E[R][G][P], EB[R];
    auto load = [&](float (&Er)[G][P], float& eb, int t0) {
        const int Tc = T > 0 ? T - 1 : 0;
        eb = em[(size_t)min(t0 + (lane < G ? lane : 0), Tc) * pitch];
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const float* src = em + (size_t)min(t0 + u, Tc) * pitch;
#pragma unroll
            for (int i = 0; i < P; ++i) Er[u][i] = src[col[i]];
        }
    };

    auto step = [&](const float (&Eu)[P], float eb, int t) __attribute__((always_inline)) {
        float lm1 = from_lane_below(lb[P - 1]);
        if (NW > 1) {
            if (lane == 63) xl[t & 1][wave] = lb[P - 1];
            __syncthreads();
            if (lane == 0 && wave > 0) lm1 = xl[t & 1][wave - 1];
        }
        float nb[P], nl[P];
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const float lp = i == 0 ? lm1 : lb[i > 0 ? i - 1 : 0];
            nb[i] = eb + lse2(bl[i], lp);
            const float el = lvalid[i] ? Eu[i] : neg_inf();
            nl[i] = el + lse3(lb[i], bl[i], allow[i] ? lp : neg_inf());
        }
#pragma unroll
        for (int i = 0; i < P; ++i) {
            bl[i] = nb[i];
            lb[i] = nl[i];
        }
        if ((t & (kRebase - 1)) == kRebase - 1) {             // uniform over the workgroup
            float m = neg_inf();
#pragma unroll
            for (int i = 0; i < P; ++i) m = fmaxf(m, fmaxf(bl[i], lb[i]));
            m = hfa::wave_max(m);
            if (NW > 1) {
                const int slot = (t / kRebase) & 1;
                if (lane == 0) red[slot][wave] = m;
                __syncthreads();
#pragma unroll
                for (int w = 0; w < NW; ++w) m = fmaxf(m, red[slot][w]);
            }
            const float sub = m == neg_inf() ? 0.0f : m;      // (state 0 is always reachable: never -inf in practice)
#pragma unroll
            for (int i = 0; i < P; ++i) {
                bl[i] -= sub;
                lb[i] -= sub;
            }
            offset += (double)sub;
        }
    };

    if (T > 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) load(E[r], EB[r], r * G);
        int tb = 0;
        for (; tb + R * G <= T; tb += R * G) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int u = 0; u < G; ++u)
                    step(E[r][u], __int_as_float(__builtin_amdgcn_readlane(__float_as_int(EB[r]), u)), tb + r * G + u);
                load(E[r], EB[r], tb + (r + R) * G);          // refill this slot for the group R ahead
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int u = 0; u < G; ++u) {
                const int t = tb + r * G + u;
                if (t < T)                                    // uniform over the workgroup
                    step(E[r][u], __int_as_float(__builtin_amdgcn_readlane(__float_as_int(EB[r]), u)), t);
            }
        }
    }
    __syncthreads();                                          // fin's initialisation
#pragma unroll
    for (int i = 0; i < P; ++i) {
        if (j0 + i == L) fin[0] = bl[i];
        if (j0 + i == L - 1) fin[1] = lb[i];
    }
    __syncthreads();
    if (g == 0) {
        const double a = (double)fin[0], c = (double)fin[1];
        const double hi = a > c ? a : c, lo = a > c ? c : a;
        double out = __builtin_inf();                         // infeasible: +inf, as torch with zero_infinity=False
        if (hi > -__builtin_inf()) out = 0.0 - (offset + hi + log1p(exp(lo - hi)));
        nll[b] = out;
    }
}

// ---- greedy decode: keep frame t when best[t] != best[t-1] (best[-1] = 0) and best[t] != 0 ------------------------
__global__ __launch_bounds__(256) void ctc_greedy_kernel(int Tmax, const int32_t* __restrict__ Tv,
                                                         const int32_t* __restrict__ best, int32_t* __restrict__ ids,
                                                         int32_t* __restrict__ n_out) {
    __shared__ int warp_cnt[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = min(Tv[b], Tmax);
    const int32_t* bb = best + (size_t)b * Tmax;
    const int lane = tid & 63, w = tid >> 6;
    int base = 0;
    for (int t0 = 0; t0 < T; t0 += 256) {
        const int t = t0 + tid;
        int keep = 0, c = 0;
        if (t < T) {
            c = bb[t];
            const int p = t > 0 ? bb[t - 1] : 0;
            keep = c != p && c != 0;
        }
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) warp_cnt[w] = __popcll(m);
        __syncthreads();
        int off = base, total = 0;
        for (int i = 0; i < 4; ++i) {
            if (i < w) off += warp_cnt[i];
            total += warp_cnt[i];
        }
        if (keep) ids[(size_t)b * Tmax + off + before] = c;
        base += total;
        __syncthreads();
    }
    if (tid == 0) n_out[b] = base;
}

bool misaligned(const void* p, size_t a) { return ((uintptr_t)p % a) != 0; }

}  // namespace

extern "C" {

int hfa_ctc_max_labels(void) { return kMaxLabels; }

int hfa_ctc_prologue(int B, int Tmax, int V, int Lmax, const int32_t* T, const int32_t* L, const float* logits,
                     long long ld, long long bs, int blank_col, int label_off, const int32_t* targets, float* emis,
                     int32_t* best, hipStream_t stream) {
    if (B < 0 || Tmax < 0 || V <= 0 || V > kMaxV || Lmax < 0 || Lmax > kMaxLabels) {
        hfa::set_error("hfa_ctc_prologue: bad sizes (B, Tmax >= 0, 0 < V <= %d, 0 <= Lmax <= %d)", kMaxV, kMaxLabels);
        return HFA_EINVAL;
    }
    if (blank_col < 0 || label_off < -1 || ld < 0 || bs < 0) {
        hfa::set_error("hfa_ctc_prologue: bad layout (blank_col >= 0, label_off >= -1, strides >= 0)");
        return HFA_EINVAL;
    }
    if (B == 0 || Tmax == 0) return HFA_OK;
    if (!T || !L || !logits || !emis || !best || (Lmax > 0 && !targets)) {
        hfa::set_error("hfa_ctc_prologue: null pointer");
        return HFA_EINVAL;
    }
    if (misaligned(T, 4) || misaligned(L, 4) || misaligned(logits, 4) || misaligned(emis, 4) || misaligned(best, 4) ||
        misaligned(targets, 4)) {
        hfa::set_error("hfa_ctc_prologue: misaligned pointer (4-byte elements)");
        return HFA_EINVAL;
    }
    const int tb = (Tmax + kProThreads / 64 - 1) / (kProThreads / 64);
    const int gx = hfa::capped((long long)tb * B) / B;
    dim3 grid(gx > 0 ? gx : 1, B);
    hipLaunchKernelGGL(ctc_prologue_kernel, grid, dim3(kProThreads), 0, stream, Tmax, V, Lmax, T, L, logits, ld, bs,
                       blank_col, label_off, targets, emis, best);
    return hfa::check_launch("hfa_ctc_prologue");
}

int hfa_ctc_forward(int B, int Tmax, int Lmax, const int32_t* T, const int32_t* L, const float* emis,
                    const int32_t* targets, double* nll, hipStream_t stream) {
    if (B < 0 || Tmax < 0 || Lmax < 0 || Lmax > kMaxLabels) {
        hfa::set_error("hfa_ctc_forward: bad sizes (B, Tmax >= 0, 0 <= Lmax <= %d)", kMaxLabels);
        return HFA_EINVAL;
    }
    if (B == 0) return HFA_OK;
    if (!T || !L || !nll || (Tmax > 0 && !emis) || (Lmax > 0 && !targets)) {
        hfa::set_error("hfa_ctc_forward: null pointer");
        return HFA_EINVAL;
    }
    if (misaligned(T, 4) || misaligned(L, 4) || misaligned(emis, 4) || misaligned(targets, 4) || misaligned(nll, 8)) {
        hfa::set_error("hfa_ctc_forward: misaligned pointer (4-byte elements, nll 8)");
        return HFA_EINVAL;
    }
#define HFA_CTC(P, NW, G)                                                                                            \
    do {                                                                                                             \
        hipLaunchKernelGGL((ctc_forward_kernel<P, NW, G>), dim3(B), dim3(64 * NW), 0, stream, Tmax, Lmax, T, L, emis, \
                           targets, nll);                                                                            \
        return hfa::check_launch("hfa_ctc_forward");                                                                 \
    } while (0)
    // one wave up to 4 pairs (8 states) per lane, as the Viterbi DP; then 4 pairs per lane over 2..16 waves, 8 over 16
    const int pairs = Lmax + 1;
    if (pairs <= 64) HFA_CTC(1, 1, 8);
    if (pairs <= 128) HFA_CTC(2, 1, 8);
    if (pairs <= 256) HFA_CTC(4, 1, 8);
    if (pairs <= 512) HFA_CTC(4, 2, 8);
    if (pairs <= 1024) HFA_CTC(4, 4, 8);
    if (pairs <= 2048) HFA_CTC(4, 8, 4);
    if (pairs <= 4096) HFA_CTC(4, 16, 2);     // 1024 threads cap VGPRs at 128: shorter groups
    HFA_CTC(8, 16, 2);
#undef HFA_CTC
}

int hfa_ctc_greedy(int B, int Tmax, const int32_t* T, const int32_t* best, int32_t* ids, int32_t* n,
                   hipStream_t stream) {
    if (B < 0 || Tmax < 0) {
        hfa::set_error("hfa_ctc_greedy: bad sizes (B, Tmax >= 0)");
        return HFA_EINVAL;
    }
    if (B == 0) return HFA_OK;
    if (!T || !n || (Tmax > 0 && (!best || !ids))) {
        hfa::set_error("hfa_ctc_greedy: null pointer");
        return HFA_EINVAL;
    }
    if (misaligned(T, 4) || misaligned(best, 4) || misaligned(ids, 4) || misaligned(n, 4)) {
        hfa::set_error("hfa_ctc_greedy: misaligned pointer (4-byte elements)");
        return HFA_EINVAL;
    }
    hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(256), 0, stream, Tmax, T, best, ids, n);
    return hfa::check_launch("hfa_ctc_greedy");
}

}  // extern "C"
