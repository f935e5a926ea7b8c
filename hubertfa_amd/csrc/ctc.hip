// ctc.hip — the CTC head's device path: gathered log-softmax + argmax, batched sequence likelihood, greedy decode,
// and the forward-backward: state posteriors, the per-label report and the loss gradient.
//
// Replaces (reference, paths relative to the HubertFA repository):
//   * F.log_softmax(ctc_logits) + nn.CTCLoss(reduction="none")   networks/task/forced_alignment.py:256-272,
//                                                                networks/loss/GHMLoss.py:12-56  -> hfa_ctc_prologue,
//                                                                                                   hfa_ctc_forward
//   * AlignmentDecoder.ctc (argmax + collapse)                   tools/alignment_decoder.py:145-150 -> hfa_ctc_prologue,
//                                                                                                   hfa_ctc_greedy
//   * the backward of that nn.CTCLoss (the gradient with respect   networks/task/forced_alignment.py:256-272
//     to the head logits) and the state posterior behind it                                     -> hfa_ctc_forward_alpha,
//                                                                                                   hfa_ctc_backward,
//                                                                                                   hfa_ctc_grad
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

#include <type_traits>

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

// base[idx] with a 32-bit byte offset, so a uniform base can stay in SGPRs with the lane's part in one VGPR
template <typename T>
__device__ __forceinline__ T* at32(T* base, int idx) {
    using C = std::conditional_t<std::is_const_v<T>, const char, char>;
    return reinterpret_cast<T*>(reinterpret_cast<C*>(base) + (unsigned)idx * (unsigned)sizeof(T));
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
// kStore (hfa_ctc_forward_alpha): every step's alpha row, after its rebase, goes to alpha [B,Tmax,2,Lmax+1] (plane 0
// the blanks j <= L, plane 1 the labels j < L; plane 1's slot L, which no state owns, takes the stores of the pairs
// past L and holds garbage) and the offset it is relative to to aoff [B,Tmax]; the stores are off the scan's
// dependency chain and the arithmetic is the plain form's, so nll has the same bits.
template <int P, int NW, int G, bool kStore>
__global__ __launch_bounds__(64 * NW) void ctc_forward_kernel(
    int Tmax, int Lmax, const int32_t* __restrict__ Tv, const int32_t* __restrict__ Lv,
    const float* __restrict__ emis, const int32_t* __restrict__ targets, double* __restrict__ nll,
    float* __restrict__ alpha, double* __restrict__ aoff) {
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
        if constexpr (kStore) {
            float* ar = alpha + ((size_t)b * Tmax + t) * 2 * pitch;
#pragma unroll
            for (int i = 0; i < P; ++i) {
                if (NW < 16) {                                // no exec juggling: pairs past L all write the label
                    *at32(ar, j0 + i <= L ? j0 + i : pitch + L) = bl[i];      // plane's spare slot L
                    *at32(ar, pitch + min(j0 + i, L)) = lb[i];
                } else {                                      // (128 VGPRs: the clamped offsets would spill)
                    if (j0 + i <= L) *at32(ar, j0 + i) = bl[i];
                    if (lvalid[i]) *at32(ar, pitch + j0 + i) = lb[i];
                }
            }
            if (g == 0) aoff[(size_t)b * Tmax + t] = offset;
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

// ---- backward: beta, the state posterior gamma and the per-label summaries ---------------------------------------
// The mirror scan, t = T - 1 down to 0 (k = T - 1 - t counts the steps), on the forward's tiling.  With e as above and
// beta including its own frame's emission (torch's convention):
//     b_j' = e[0]     + lse(b_j, l_j)
//     l_j' = e[j + 1] + lse(l_j, b_{j+1}, l_{j+1} if target j+1 != target j)
// so what crosses lanes is the blank and the label of the pair above (two DPP moves the other way; two LDS slots
// across waves).  The virtual row after frame T - 1 has all mass on blank_L.  beta is rebased after every step with
// k % 16 == 15, as alpha.  Each step reads the stored alpha row (prefetched with the emissions) and forms
//     gamma = exp(f32(alpha_rel + beta_rel - e) + f32(aoff[t] + (boff + nll)))          (0 where either is -inf)
// writes the labels' gamma to occ and accumulates frames / centre / logp in the registers of the label's lane, in
// descending t whatever the form.  Column 0 is the sum of the blanks' gamma over a FIXED binary tree on the pair index
// (within the lane, then the lanes in blocks of 2, 4, .. 64, then the waves pairwise), so it too has the same bits in
// every form: the absent pairs of a wider form add exact zeros.
__device__ __forceinline__ float from_lane_above(float v) {   // DPP wave_shl:1, lane 63 receives -inf
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(neg_inf()), __float_as_int(v), 0x130, 0xF, 0xF,
                                                      false));
}

// The wave's sum over the fixed tree: lanes by xor 1, 2 (quad permutes), 4, 8 (row half mirror / mirror: the partner
// holds the other half's sum), then the four rows' sums pairwise.  No LDS round trips; the same value in every lane.
template <int kCtrl>
__device__ __forceinline__ float add_dpp(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, 0xF, 0xF, false));
}
__device__ __forceinline__ float tree_over_lanes(float v) {
    v = add_dpp<0xB1>(v);                                     // quad_perm [1,0,3,2]
    v = add_dpp<0x4E>(v);                                     // quad_perm [2,3,0,1]
    v = add_dpp<0x141>(v);                                    // row_half_mirror
    v = add_dpp<0x140>(v);                                    // row_mirror
    auto row = [&](int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); };
    return (row(0) + row(16)) + (row(32) + row(48));
}

template <int NW>
__device__ __forceinline__ float tree_over_waves(const float* v) {
    float w[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = v[i];
#pragma unroll
    for (int s = 1; s < NW; s <<= 1) {
#pragma unroll
        for (int i = 0; i < NW; i += 2 * s) w[i] += w[i + s];
    }
    return w[0];
}

template <int P, int NW, int G>
__global__ __launch_bounds__(64 * NW) void ctc_backward_kernel(
    int Tmax, int Lmax, const int32_t* __restrict__ Tv, const int32_t* __restrict__ Lv,
    const float* __restrict__ emis, const int32_t* __restrict__ targets, const double* __restrict__ nllv,
    const float* __restrict__ alpha, const double* __restrict__ aoff, float* __restrict__ occ,
    float* __restrict__ frames, float* __restrict__ centre, float* __restrict__ logp) {
    static_assert(G <= 64 && kRebase % G == 0, "a group's blank emissions fit one wave's lanes");
    constexpr int R = 2;
    __shared__ float xb[2][NW], xl[2][NW];   // a wave's first blank / label, for lane 63 of the wave below
    __shared__ float red[2][NW];             // rebase: the waves' maxima
    __shared__ float cs[2][NW];              // the waves' sums of the blanks' gamma
    const int b = blockIdx.x;
    const int g = threadIdx.x;
    const int lane = g & 63, wave = g >> 6;
    const int T = min(Tv[b], Tmax);
    const int L = min(Lv[b], Lmax);
    const int pitch = Lmax + 1;
    const float* em = emis + (size_t)b * Tmax * pitch;
    const float* al = alpha + (size_t)b * Tmax * 2 * pitch;
    const double* ao = aoff + (size_t)b * Tmax;
    float* oc = occ + (size_t)b * Tmax * pitch;
    const int32_t* tg = targets + (size_t)b * Lmax;
    const double nll = nllv[b];
    const bool feasible = nll < __builtin_inf();
    const int j0 = g * P;

    for (int t = wave; t < Tmax; t += NW) {                   // zeros past the row's own frames and labels
        for (int j = ((t < T && feasible) ? L + 1 : 0) + lane; j < pitch; j += 64) oc[(size_t)t * pitch + j] = 0.0f;
    }
    if (!feasible) {                                          // uniform over the workgroup
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const int j = j0 + i;
            if (j < Lmax) {
                frames[(size_t)b * Lmax + j] = 0.0f;
                centre[(size_t)b * Lmax + j] = 0.0f;
                logp[(size_t)b * Lmax + j] = j < L ? neg_inf() : 0.0f;
            }
        }
        return;
    }

    float bl[P], lb[P];                  // beta of the blank / label state of this lane's pairs
    float fr[P], ce[P], lp[P];           // sum_t gamma, sum_t t gamma, sum_t gamma e of the label
    bool lvalid[P], allowup[P];
    int col[P], acol[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int j = j0 + i;
        lvalid[i] = j < L;
        col[i] = lvalid[i] ? j + 1 : 0;                       // clamped, as the forward
        acol[i] = min(j, L);
        const int cur = lvalid[i] ? tg[j] : 0;
        const int nxt = j + 1 < L ? tg[j + 1] : 0;
        allowup[i] = j + 1 < L && nxt != cur;
        bl[i] = j == L ? 0.0f : neg_inf();                    // the virtual row after frame T - 1
        lb[i] = neg_inf();
        fr[i] = ce[i] = lp[i] = 0.0f;
    }
    double boff = 0.0;

    float E[R][G][P], AB[R][G][P], AL[R][G][P], EB[R];
    double AO[R];
    auto load = [&](float (&Er)[G][P], float (&Ab)[G][P], float (&Al)[G][P], float& eb, double& a0, int k0) {
        const int Tc = T > 0 ? T - 1 : 0;
        const int tl = Tc - min(k0 + (lane < G ? lane : 0), Tc);
        eb = em[(size_t)tl * pitch];
        a0 = ao[tl];
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const size_t t = (size_t)(Tc - min(k0 + u, Tc));
            const float* src = em + t * pitch;
            const float* as = al + t * 2 * pitch;
#pragma unroll
            for (int i = 0; i < P; ++i) {
                Er[u][i] = *at32(src, col[i]);
                Ab[u][i] = *at32(as, acol[i]);
                Al[u][i] = *at32(as, pitch + acol[i]);
            }
        }
    };

    auto step = [&](const float (&Eu)[P], const float (&Ab)[P], const float (&Al)[P], float eb, double a0, int k)
                    __attribute__((always_inline)) {
        const int t = T - 1 - k;
        float bup = from_lane_above(bl[0]), lup = from_lane_above(lb[0]);
        if (NW > 1) {
            if (lane == 0) {
                xb[k & 1][wave] = bl[0];
                xl[k & 1][wave] = lb[0];
            }
            __syncthreads();
            if (lane == 63 && wave < NW - 1) {
                bup = xb[k & 1][wave + 1];
                lup = xl[k & 1][wave + 1];
            }
            if (g == 0 && k > 0) oc[(size_t)(t + 1) * pitch] = tree_over_waves<NW>(cs[(k - 1) & 1]);
        }
        float nb[P], nl[P];
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const float bn = i == P - 1 ? bup : bl[i < P - 1 ? i + 1 : 0];
            const float ln = i == P - 1 ? lup : lb[i < P - 1 ? i + 1 : 0];
            nb[i] = eb + lse2(bl[i], lb[i]);
            const float el = lvalid[i] ? Eu[i] : neg_inf();
            nl[i] = el + lse3(lb[i], bn, allowup[i] ? ln : neg_inf());
        }
#pragma unroll
        for (int i = 0; i < P; ++i) {
            bl[i] = nb[i];
            lb[i] = nl[i];
        }
        if ((k & (kRebase - 1)) == kRebase - 1) {             // uniform over the workgroup
            float m = neg_inf();
#pragma unroll
            for (int i = 0; i < P; ++i) m = fmaxf(m, fmaxf(bl[i], lb[i]));
            m = hfa::wave_max(m);
            if (NW > 1) {
                const int slot = (k / kRebase) & 1;
                if (lane == 0) red[slot][wave] = m;
                __syncthreads();
#pragma unroll
                for (int w = 0; w < NW; ++w) m = fmaxf(m, red[slot][w]);
            }
            const float sub = m == neg_inf() ? 0.0f : m;
#pragma unroll
            for (int i = 0; i < P; ++i) {
                bl[i] -= sub;
                lb[i] -= sub;
            }
            boff += (double)sub;
        }
        // gamma: off the scan's dependency chain
        const float c = (float)(a0 + (boff + nll));
        float gb[P];
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const bool zb = Ab[i] == neg_inf() || bl[i] == neg_inf();
            gb[i] = zb ? 0.0f : expf(((Ab[i] + bl[i]) - eb) + c);
            const bool zl = Al[i] == neg_inf() || lb[i] == neg_inf();
            const float gl = zl ? 0.0f : expf(((Al[i] + lb[i]) - Eu[i]) + c);
            if (lvalid[i]) *at32(oc + (size_t)t * pitch, j0 + i + 1) = gl;
            fr[i] += gl;
            ce[i] += (float)t * gl;
            lp[i] += zl ? 0.0f : gl * Eu[i];
        }
#pragma unroll
        for (int s = 1; s < P; s <<= 1) {
#pragma unroll
            for (int i = 0; i < P; i += 2 * s) gb[i] += gb[i + s];
        }
        const float sb = tree_over_lanes(gb[0]);
        if (NW > 1) {
            if (lane == 0) cs[k & 1][wave] = sb;
        } else if (lane == 0) {
            oc[(size_t)t * pitch] = sb;
        }
    };

    auto rl = [](float v, int u) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), u)); };
    auto rld = [](double v, int u) {
        return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), u),
                                __builtin_amdgcn_readlane(__double2loint(v), u));
    };
    if (T > 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) load(E[r], AB[r], AL[r], EB[r], AO[r], r * G);
        int kb = 0;
        for (; kb + R * G <= T; kb += R * G) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int u = 0; u < G; ++u)
                    step(E[r][u], AB[r][u], AL[r][u], rl(EB[r], u), rld(AO[r], u), kb + r * G + u);
                load(E[r], AB[r], AL[r], EB[r], AO[r], kb + (r + R) * G);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int u = 0; u < G; ++u) {
                const int k = kb + r * G + u;
                if (k < T)                                    // uniform over the workgroup
                    step(E[r][u], AB[r][u], AL[r][u], rl(EB[r], u), rld(AO[r], u), k);
            }
        }
        if (NW > 1) {
            __syncthreads();
            if (g == 0) oc[0] = tree_over_waves<NW>(cs[(T - 1) & 1]);
        }
    }
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int j = j0 + i;
        if (j < Lmax) {
            frames[(size_t)b * Lmax + j] = lvalid[i] ? fr[i] : 0.0f;
            centre[(size_t)b * Lmax + j] = lvalid[i] ? ce[i] / fr[i] : 0.0f;
            logp[(size_t)b * Lmax + j] = lvalid[i] ? lp[i] / fr[i] : 0.0f;
        }
    }
}

// ---- gradient: one wave per frame row ---------------------------------------------------------------------------
// grad[t, c] = w (softmax(x[t])[c] - Gamma[t, c]); Gamma of the blank is occ's column 0, Gamma of class c the sum of
// occ's columns of the target positions cls_idx[cls_ptr[c] .. cls_ptr[c + 1]) in that order (no atomics: the same
// bits alone and in a batch).  Rows t >= T[b] and every row of an infeasible utterance are zeros.
__global__ __launch_bounds__(kProThreads) void ctc_grad_kernel(
    int Tmax, int V, int Lmax, const int32_t* __restrict__ Tv, const int32_t* __restrict__ Lv,
    const float* __restrict__ logits, long long ld, long long bs, int blank_col, int label_off,
    const float* __restrict__ occ, const double* __restrict__ nllv, const int32_t* __restrict__ cls_ptr,
    const int32_t* __restrict__ cls_idx, const float* __restrict__ weight, float* __restrict__ grad, long long g_ld,
    long long g_bs) {
    __shared__ float xs[kProThreads / 64][kMaxV];
    const int b = blockIdx.y;
    const int T = nllv[b] < __builtin_inf() ? min(Tv[b], Tmax) : 0;
    const int L = min(Lv[b], Lmax);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* xw = xs[w];
    const int32_t* cp = cls_ptr + (size_t)b * (V + 1);
    const int32_t* ci = cls_idx + (size_t)b * Lmax;
    const float wt = weight ? weight[b] : 1.0f;
    const int tstride = gridDim.x * (kProThreads / 64);
    for (int t = blockIdx.x * (kProThreads / 64) + w; t < Tmax; t += tstride) {
        float* gr = grad + b * g_bs + t * g_ld;
        if (t >= T) {                                         // uniform over the wave; such logit rows are never read
            for (int c = lane; c < V; c += 64) gr[c == 0 ? blank_col : c + label_off] = 0.0f;
            continue;
        }
        const float* xr = logits + b * bs + t * ld;
        float m = neg_inf();
        for (int c = lane; c < V; c += 64) {
            const float x = xr[c == 0 ? blank_col : c + label_off];
            xw[c] = x;
            m = fmaxf(m, x);
        }
        m = hfa::wave_max(m);
        float sum = 0.0f;
        for (int c = lane; c < V; c += 64) sum += expf(xw[c] - m);
        sum = hfa::wave_sum(sum);
        const float lse = logf(sum);
        const float* orow = occ + ((size_t)b * Tmax + t) * (Lmax + 1);
        for (int c = lane; c < V; c += 64) {
            float G = 0.0f;
            if (c == 0) {
                G = orow[0];
            } else {
                const int k1 = min(cp[c + 1], L);
                for (int k = max(cp[c], 0); k < k1; ++k) G += orow[min(max(ci[k], 0), L - 1) + 1];
            }
            gr[c == 0 ? blank_col : c + label_off] = wt * (expf((xw[c] - m) - lse) - G);
        }
        __builtin_amdgcn_wave_barrier();
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

// one wave up to 4 pairs (8 states) per lane, as the Viterbi DP; then 4 pairs per lane over 2..16 waves, 8 over 16
template <bool kStore>
int launch_forward(int B, int Tmax, int Lmax, const int32_t* T, const int32_t* L, const float* emis,
                   const int32_t* targets, double* nll, float* alpha, double* aoff, hipStream_t stream,
                   const char* what) {
#define HFA_CTC(P, NW, G)                                                                                            \
    do {                                                                                                             \
        hipLaunchKernelGGL((ctc_forward_kernel<P, NW, G, kStore>), dim3(B), dim3(64 * NW), 0, stream, Tmax, Lmax, T, \
                           L, emis, targets, nll, alpha, aoff);                                                      \
        return hfa::check_launch(what);                                                                              \
    } while (0)
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
    return launch_forward<false>(B, Tmax, Lmax, T, L, emis, targets, nll, nullptr, nullptr, stream, "hfa_ctc_forward");
}

int hfa_ctc_forward_alpha(int B, int Tmax, int Lmax, const int32_t* T, const int32_t* L, const float* emis,
                          const int32_t* targets, double* nll, float* alpha, double* aoff, hipStream_t stream) {
    if (B < 0 || Tmax < 0 || Lmax < 0 || Lmax > kMaxLabels) {
        hfa::set_error("hfa_ctc_forward_alpha: bad sizes (B, Tmax >= 0, 0 <= Lmax <= %d)", kMaxLabels);
        return HFA_EINVAL;
    }
    if (B == 0) return HFA_OK;
    if (!T || !L || !nll || (Tmax > 0 && (!emis || !alpha || !aoff)) || (Lmax > 0 && !targets)) {
        hfa::set_error("hfa_ctc_forward_alpha: null pointer");
        return HFA_EINVAL;
    }
    if (misaligned(T, 4) || misaligned(L, 4) || misaligned(emis, 4) || misaligned(targets, 4) || misaligned(nll, 8) ||
        misaligned(alpha, 4) || misaligned(aoff, 8)) {
        hfa::set_error("hfa_ctc_forward_alpha: misaligned pointer (4-byte elements, nll / aoff 8)");
        return HFA_EINVAL;
    }
    return launch_forward<true>(B, Tmax, Lmax, T, L, emis, targets, nll, alpha, aoff, stream, "hfa_ctc_forward_alpha");
}

int hfa_ctc_backward(int B, int Tmax, int Lmax, const int32_t* T, const int32_t* L, const float* emis,
                     const int32_t* targets, const double* nll, const float* alpha, const double* aoff, float* occ,
                     float* frames, float* centre, float* logp, hipStream_t stream) {
    if (B < 0 || Tmax < 0 || Lmax < 0 || Lmax > kMaxLabels) {
        hfa::set_error("hfa_ctc_backward: bad sizes (B, Tmax >= 0, 0 <= Lmax <= %d)", kMaxLabels);
        return HFA_EINVAL;
    }
    if (B == 0) return HFA_OK;
    if (!T || !L || !nll || (Tmax > 0 && (!emis || !alpha || !aoff || !occ)) ||
        (Lmax > 0 && (!targets || !frames || !centre || !logp))) {
        hfa::set_error("hfa_ctc_backward: null pointer");
        return HFA_EINVAL;
    }
    if (misaligned(T, 4) || misaligned(L, 4) || misaligned(emis, 4) || misaligned(targets, 4) || misaligned(nll, 8) ||
        misaligned(alpha, 4) || misaligned(aoff, 8) || misaligned(occ, 4) || misaligned(frames, 4) ||
        misaligned(centre, 4) || misaligned(logp, 4)) {
        hfa::set_error("hfa_ctc_backward: misaligned pointer (4-byte elements, nll / aoff 8)");
        return HFA_EINVAL;
    }
#define HFA_CTC(P, NW, G)                                                                                             \
    do {                                                                                                              \
        hipLaunchKernelGGL((ctc_backward_kernel<P, NW, G>), dim3(B), dim3(64 * NW), 0, stream, Tmax, Lmax, T, L, emis, \
                           targets, nll, alpha, aoff, occ, frames, centre, logp);                                     \
        return hfa::check_launch("hfa_ctc_backward");                                                                 \
    } while (0)
    // the forward's forms; three prefetched arrays instead of one, so the groups are half as long past 1 pair per lane
    const int pairs = Lmax + 1;
    if (pairs <= 64) HFA_CTC(1, 1, 8);
    if (pairs <= 128) HFA_CTC(2, 1, 4);
    if (pairs <= 256) HFA_CTC(4, 1, 4);
    if (pairs <= 512) HFA_CTC(4, 2, 4);
    if (pairs <= 1024) HFA_CTC(4, 4, 4);
    if (pairs <= 2048) HFA_CTC(4, 8, 2);
    if (pairs <= 4096) HFA_CTC(4, 16, 1);
    HFA_CTC(8, 16, 1);
#undef HFA_CTC
}

int hfa_ctc_grad(int B, int Tmax, int V, int Lmax, const int32_t* T, const int32_t* L, const float* logits,
                 long long ld, long long bs, int blank_col, int label_off, const float* occ, const double* nll,
                 const int32_t* cls_ptr, const int32_t* cls_idx, const float* weight, float* grad, long long g_ld,
                 long long g_bs, hipStream_t stream) {
    if (B < 0 || Tmax < 0 || V <= 0 || V > kMaxV || Lmax < 0 || Lmax > kMaxLabels) {
        hfa::set_error("hfa_ctc_grad: bad sizes (B, Tmax >= 0, 0 < V <= %d, 0 <= Lmax <= %d)", kMaxV, kMaxLabels);
        return HFA_EINVAL;
    }
    if (blank_col < 0 || label_off < -1 || ld < 0 || bs < 0 || g_ld < 0 || g_bs < 0) {
        hfa::set_error("hfa_ctc_grad: bad layout (blank_col >= 0, label_off >= -1, strides >= 0)");
        return HFA_EINVAL;
    }
    if (B == 0 || Tmax == 0) return HFA_OK;
    if (!T || !L || !logits || !occ || !nll || !cls_ptr || !grad || (Lmax > 0 && !cls_idx)) {
        hfa::set_error("hfa_ctc_grad: null pointer");
        return HFA_EINVAL;
    }
    if (misaligned(T, 4) || misaligned(L, 4) || misaligned(logits, 4) || misaligned(occ, 4) || misaligned(nll, 8) ||
        misaligned(cls_ptr, 4) || misaligned(cls_idx, 4) || misaligned(weight, 4) || misaligned(grad, 4)) {
        hfa::set_error("hfa_ctc_grad: misaligned pointer (4-byte elements, nll 8)");
        return HFA_EINVAL;
    }
    const int tb = (Tmax + kProThreads / 64 - 1) / (kProThreads / 64);
    const int gx = hfa::capped((long long)tb * B) / B;
    dim3 grid(gx > 0 ? gx : 1, B);
    hipLaunchKernelGGL(ctc_grad_kernel, grid, dim3(kProThreads), 0, stream, Tmax, V, Lmax, T, L, logits, ld, bs,
                       blank_col, label_off, occ, nll, cls_ptr, cls_idx, weight, grad, g_ld, g_bs);
    return hfa::check_launch("hfa_ctc_grad");
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
