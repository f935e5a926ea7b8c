// loss.hip — the four full-label alignment losses of the reference's _get_loss, fused, with their gradient with
// respect to the head logits and the statistics the reference's EMA tables are updated from.
//
// Replaces (reference, paths relative to the HubertFA repository), for the rows with label_type >= 2 of
// networks/task/forced_alignment.py:188-254:
//   * ph_frame_GHM_loss   GHMLoss, networks/loss/GHMLoss.py:221-302            -> hfa_fa_frame_loss (term 0)
//   * ph_edge_GHM_loss    MultiLabelGHMLoss(1), GHMLoss.py:117-211             -> hfa_fa_frame_loss (term 1)
//   * ph_edge_diff_loss   the same class on forced_alignment.py:224-236's pairs -> hfa_fa_frame_loss (term 2)
//   * ph_edge_EMD_loss    BinaryEMDLoss, networks/loss/BinaryEMDLoss.py:4-15   -> hfa_fa_emd
//   * the sums, the normalisers and the bincounts of GHMLoss.py:181-209, :278-300 -> hfa_fa_loss_reduce
//
// The head's layout: column 0 of a frame's V + 2 logits is the edge, column 1 the CTC blank (never read or written
// here), columns 2.. the V frame classes.  m[b,t] = t < T[b]; a row takes part iff label_type[b] >= 2.
//
// Frame term (GHMLoss.py:253-276): class c is live iff ph_mask[b,c] and m[b,t]; the reference's x - 1e9 on dead classes
// is an exact zero probability in f32, so dead classes are left out of the max, the sum and the target; target_c =
// clamp(onehot, f32(ls), f32(1 - ls)) on live classes (the reference's .float() one-hot; it does not sum to 1: d raw /
// d x_c = (sum target) softmax_c - target_c); GD = |softmax[label] - target[label]|; weight = sqrt(class_ema[label]
// GD_ema[bin]), a constant for the gradient.
// Edge term (GHMLoss.py:161-179): BCEWithLogits on the raw edge logit, weight sqrt((1 / GD_stat_ema[bin] + 1e-3)
// (1 / label_stat_ema_each_class[floor(3 target)] + 1e-3)).  Difference term: the same on z = (sigmoid(x[t+1]) -
// sigmoid(x[t]) + 1) / 2, fed as if it were a logit, against (gt[t+1] - gt[t] + 1) / 2, for t + 1 < T[b]; frame t's
// edge logit gets gradient from pair t - 1 and pair t, both formed by the wave that owns frame t: no atomics.
// EMD term: d_t = (sigmoid(x_t) - gt_t) m_t; loss = (mean_u |F_u| + mean_u |R_u|) / 2 over all Tmax columns, F / R the
// forward / reverse inclusive cumulative sums; for u >= T the forward sum stays sum(d) and the reverse one is 0.
//
// Determinism: no float atomics.  Every per-frame value depends on its own frame (and its two neighbours' edge logits)
// only; the scans and the reductions run over fixed trees on the frame index, so a row has the same bits alone, in a
// batch and under any grid cap.  Built with -ffp-contract=off, as ctc.hip.
#include "hfa_common.h"

namespace {

using hfa::neg_inf;

constexpr int kMaxV = 1024;             // as hfa_ctc_prologue
constexpr int kMaxBins = 64;
constexpr int kRowThreads = 256;        // four waves, one frame row each
constexpr int kScanThreads = 256;
constexpr int kScanK = 4;               // consecutive frames per lane
constexpr int kScanTile = kScanThreads * kScanK;

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }
// BCEWithLogits, reduction none
__device__ __forceinline__ float bce_logits(float x, float g) {
    return (fmaxf(x, 0.0f) - x * g) + log1pf(expf(-fabsf(x)));
}
__device__ __forceinline__ int bin_of(float v, int n) { return min(max((int)floorf(v), 0), n - 1); }

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One GHM-weighted BCE sample of MultiLabelGHMLoss(1): the weighted loss, d loss / d logit, and the two bins.
struct EdgeSample {
    float term, dterm;
    int gd_bin, lab_bin;
};
__device__ __forceinline__ EdgeSample edge_sample(float x, float g, int nb, const float* __restrict__ gd_ema,
                                                  const float* __restrict__ lab_ema) {
    EdgeSample s;
    const float p = sigmoid_f(x);
    s.gd_bin = bin_of(fabsf(p - g) * (float)nb, nb);
    s.lab_bin = bin_of(g * 3.0f, 3);
    const float w = sqrtf((1.0f / gd_ema[s.gd_bin] + 1e-3f) * (1.0f / lab_ema[s.lab_bin] + 1e-3f));
    s.term = bce_logits(x, g) * w;
    s.dterm = w * (p - g);
    return s;
}

// ---- the three per-frame terms: one wave per frame row ------------------------------------------------------------
__global__ __launch_bounds__(kRowThreads) void fa_frame_kernel(
    int Tmax, int V, int nb, float ls, float hs, const int32_t* __restrict__ Tv, const int32_t* __restrict__ ltv,
    const float* __restrict__ logits, long long ld, long long bs, const int32_t* __restrict__ ph_frame,
    const float* __restrict__ ph_edge, const int32_t* __restrict__ ph_mask, const float* __restrict__ tables,
    float* __restrict__ terms, int32_t* __restrict__ bins, const float* __restrict__ coef,
    const int32_t* __restrict__ emd_fac, float* __restrict__ grad, long long g_ld, long long g_bs) {
    __shared__ float xs[kRowThreads / 64][kMaxV];
    const int b = blockIdx.y;
    const int T = ltv[b] >= 2 ? min(max(Tv[b], 0), Tmax) : 0;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* xw = xs[w];
    const float* class_ema = tables;
    const float* gd_ema = class_ema + V;
    const float* egd = gd_ema + nb;
    const float* elab = egd + nb;
    const float* dgd = elab + 3;
    const float* dlab = dgd + nb;
    const int32_t* mk = ph_mask + (size_t)b * V;
    const float* e0 = logits + b * bs;                         // the edge column
    const float c_frame = grad ? coef[0] : 0.0f, c_edge = grad ? coef[1] : 0.0f, c_emd = grad ? coef[2] : 0.0f,
                c_diff = grad ? coef[3] : 0.0f;
    const int tstride = gridDim.x * (kRowThreads / 64);
    for (int t = blockIdx.x * (kRowThreads / 64) + w; t < Tmax; t += tstride) {
        const size_t ft = (size_t)b * Tmax + t;
        float* gr = grad ? grad + b * g_bs + t * g_ld : nullptr;
        if (t >= T) {                                         // uniform over the wave; such frames are never read
            if (lane < 3) terms[ft * 3 + lane] = 0.0f;
            if (lane < 5) bins[ft * 5 + lane] = -1;
            if (gr) {
                if (lane == 0) gr[0] = 0.0f;
                for (int c = lane; c < V; c += 64) gr[2 + c] = 0.0f;
            }
            continue;
        }
        // -- frame term
        const float* xr = e0 + t * ld + 2;
        const int label = min(max(ph_frame[ft], 0), V - 1);
        float m = neg_inf();
        int nlive = 0;
        for (int c = lane; c < V; c += 64) {
            const bool live = mk[c] != 0;
            const float x = live ? xr[c] : neg_inf();          // a dead class's logit reaches nothing
            xw[c] = x;
            m = fmaxf(m, x);
            nlive += live ? 1 : 0;
        }
        m = hfa::wave_max(m);
        nlive = wave_sum_i(nlive);
        __builtin_amdgcn_wave_barrier();
        float term_f = 0.0f, gscale = 0.0f, lse = 0.0f, S = 0.0f;
        int bin_f = -1;
        const bool label_live = mk[label] != 0;
        if (nlive > 0) {                                      // uniform over the wave
            float sum = 0.0f;
            for (int c = lane; c < V; c += 64) sum += xw[c] == neg_inf() ? 0.0f : expf(xw[c] - m);
            sum = hfa::wave_sum(sum);
            lse = logf(sum);
            float acc = 0.0f;
            for (int c = lane; c < V; c += 64) {
                const float tg = c == label ? hs : ls;
                acc += xw[c] == neg_inf() ? 0.0f : tg * ((xw[c] - m) - lse);
            }
            const float raw = 0.0f - hfa::wave_sum(acc);
            const float p_lab = label_live ? expf((xw[label] - m) - lse) : 0.0f;
            const float t_lab = label_live ? hs : 0.0f;
            bin_f = bin_of(fabsf(p_lab - t_lab) * (float)nb, nb);
            const float wgt = sqrtf(class_ema[label] * gd_ema[bin_f]);
            term_f = raw / wgt;
            gscale = c_frame / wgt;
            S = label_live ? hs + (float)(nlive - 1) * ls : (float)nlive * ls;
        }
        // -- edge and edge-difference terms (the same values in every lane)
        const float x0 = e0[t * ld], g0 = ph_edge[ft];
        const EdgeSample es = edge_sample(x0, g0, nb, egd, elab);
        const float p0 = sigmoid_f(x0);
        const float dp0 = p0 * (1.0f - p0);
        float g_edge = c_edge * es.dterm;
        float term_d = 0.0f;
        int bin_dg = -1, bin_dl = -1;
        if (t + 1 < T) {                                      // pair t: frames t, t + 1
            const float p1 = sigmoid_f(e0[(t + 1) * ld]);
            const float z = ((p1 - p0) + 1.0f) * 0.5f, g = ((ph_edge[ft + 1] - g0) + 1.0f) * 0.5f;
            const EdgeSample ds = edge_sample(z, g, nb, dgd, dlab);
            term_d = ds.term;
            bin_dg = ds.gd_bin;
            bin_dl = ds.lab_bin;
            g_edge += c_diff * ds.dterm * (-0.5f * dp0);
        }
        if (gr) {
            if (t >= 1) {                                     // pair t - 1: frames t - 1, t
                const float pm = sigmoid_f(e0[(t - 1) * ld]);
                const float z = ((p0 - pm) + 1.0f) * 0.5f, g = ((g0 - ph_edge[ft - 1]) + 1.0f) * 0.5f;
                const EdgeSample ds = edge_sample(z, g, nb, dgd, dlab);
                g_edge += c_diff * ds.dterm * (0.5f * dp0);
            }
            if (emd_fac) g_edge += c_emd * dp0 * (float)emd_fac[ft];
            if (lane == 0) gr[0] = g_edge;
            for (int c = lane; c < V; c += 64) {
                float g = 0.0f;
                if (nlive > 0 && xw[c] != neg_inf()) {
                    const float tg = c == label ? hs : ls;
                    g = gscale * (S * expf((xw[c] - m) - lse) - tg);
                }
                gr[2 + c] = g;
            }
        }
        if (lane == 0) {
            terms[ft * 3 + 0] = term_f;
            terms[ft * 3 + 1] = es.term;
            terms[ft * 3 + 2] = term_d;
            bins[ft * 5 + 0] = bin_f;
            bins[ft * 5 + 1] = es.gd_bin;
            bins[ft * 5 + 2] = es.lab_bin;
            bins[ft * 5 + 3] = bin_dg;
            bins[ft * 5 + 4] = bin_dl;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- EMD: one workgroup per row ----------------------------------------------------------------------------------
// Inclusive scans over the row's T frames in tiles of 1024 with a carry: 4 consecutive frames within a lane, the lanes'
// totals by DPP row shifts and the four rows' totals over the wave, the waves' totals through LDS.  d and its sums are
// f64 (sigmoid evaluated in f64), so a 3000-frame row's cumulative sums keep every bit the f32 logits give them.
template <int kCtrl>
__device__ __forceinline__ int dpp_i(int v) {                 // lanes without a source receive 0
    return __builtin_amdgcn_update_dpp(0, v, kCtrl, 0xF, 0xF, false);
}
template <int kCtrl>
__device__ __forceinline__ double dpp_d(double v) {
    return __hiloint2double(dpp_i<kCtrl>(__double2hiint(v)), dpp_i<kCtrl>(__double2loint(v)));
}
__device__ __forceinline__ double readlane_d(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                            __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double wave_scan_d(double v, int lane) {   // inclusive, every lane active
    v += dpp_d<0x111>(v);                                     // row_shr:1, 2, 4, 8
    v += dpp_d<0x112>(v);
    v += dpp_d<0x114>(v);
    v += dpp_d<0x118>(v);
    const double r0 = readlane_d(v, 15), r1 = readlane_d(v, 31), r2 = readlane_d(v, 47);
    const int row = lane >> 4;
    return v + (row == 0 ? 0.0 : row == 1 ? r0 : row == 2 ? r0 + r1 : (r0 + r1) + r2);
}
__device__ __forceinline__ int wave_scan_i(int v, int lane) {
    v += dpp_i<0x111>(v);
    v += dpp_i<0x112>(v);
    v += dpp_i<0x114>(v);
    v += dpp_i<0x118>(v);
    const int r0 = __builtin_amdgcn_readlane(v, 15), r1 = __builtin_amdgcn_readlane(v, 31),
              r2 = __builtin_amdgcn_readlane(v, 47);
    const int row = lane >> 4;
    return v + (row == 0 ? 0 : row == 1 ? r0 : row == 2 ? r0 + r1 : r0 + r1 + r2);
}

struct ScanShared {
    double wd[2][kScanThreads / 64];
    int wi[2][kScanThreads / 64];
    double red[kScanThreads / 64];
};

// One direction's pass over the row.  Position p counts from the scan's start: frame t = p (forward) or T - 1 - p
// (reverse).  Returns through the references the sum of d, the sum of |cumulative sum| (this thread's part) and the
// sum of the signs; fac[t] receives the number of signs strictly before frame t in scan order (forward: stored;
// reverse: combined as -stored - count).
template <bool kRev>
__device__ __forceinline__ void emd_pass(int T, const float* __restrict__ e0, long long ld,
                                         const float* __restrict__ gt, int32_t* __restrict__ fac, ScanShared& sh,
                                         double& total, double& abs_part, int& sign_total) {
    const int g = threadIdx.x, lane = g & 63, wave = g >> 6;
    constexpr int NW = kScanThreads / 64;
    double carry = 0.0, acc = 0.0;
    int icarry = 0;
    int par = 0;
    for (int p0 = 0; p0 < T; p0 += kScanTile, par ^= 1) {
        double c[kScanK];
        int tt[kScanK];
        double run = 0.0;
#pragma unroll
        for (int i = 0; i < kScanK; ++i) {
            const int p = p0 + g * kScanK + i;
            const bool in = p < T;
            const int t = in ? (kRev ? T - 1 - p : p) : 0;
            tt[i] = in ? t : -1;
            double d = 0.0;
            if (in) d = 1.0 / (1.0 + exp(-(double)e0[t * ld])) - (double)gt[t];
            run += d;
            c[i] = run;
        }
        const double incl = wave_scan_d(run, lane);
        if (lane == 63) sh.wd[par][wave] = incl;
        __syncthreads();
        double before = carry, all = 0.0;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            if (k < wave) before += sh.wd[par][k];
            all += sh.wd[par][k];
        }
        before += incl - run;
        carry += all;
        int s[kScanK], srun = 0;
#pragma unroll
        for (int i = 0; i < kScanK; ++i) {
            const double C = before + c[i];
            const bool in = tt[i] >= 0;
            acc += in ? fabs(C) : 0.0;
            s[i] = in ? (C > 0.0) - (C < 0.0) : 0;
            srun += s[i];
        }
        const int iincl = wave_scan_i(srun, lane);
        if (lane == 63) sh.wi[par][wave] = iincl;
        __syncthreads();
        int ibefore = icarry, iall = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            if (k < wave) ibefore += sh.wi[par][k];
            iall += sh.wi[par][k];
        }
        ibefore += iincl - srun;
        icarry += iall;
#pragma unroll
        for (int i = 0; i < kScanK; ++i) {
            if (tt[i] >= 0) {
                if (kRev) fac[tt[i]] = 0 - fac[tt[i]] - ibefore;
                else fac[tt[i]] = ibefore;
            }
            ibefore += s[i];
        }
    }
    total = carry;
    abs_part = acc;
    sign_total = icarry;
}

__device__ __forceinline__ double block_sum_d(double v, ScanShared& sh) {   // fixed tree; the same value everywhere
    constexpr int NW = kScanThreads / 64;
    v = hfa::wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
#pragma unroll
    for (int k = 0; k < NW; ++k) r += sh.red[k];
    return r;
}

__global__ __launch_bounds__(kScanThreads) void fa_emd_kernel(
    int Tmax, const int32_t* __restrict__ Tv, const int32_t* __restrict__ ltv, const float* __restrict__ logits,
    long long ld, long long bs, const float* __restrict__ ph_edge, double* __restrict__ sums,
    int32_t* __restrict__ fac) {
    __shared__ ScanShared sh;
    const int b = blockIdx.x;
    const int T = ltv[b] >= 2 ? min(max(Tv[b], 0), Tmax) : 0;
    const float* e0 = logits + b * bs;
    const float* gt = ph_edge + (size_t)b * Tmax;
    int32_t* fr = fac + (size_t)b * Tmax;
    double totF, absF, totR, absR;
    int sF, sR;
    emd_pass<false>(T, e0, ld, gt, fr, sh, totF, absF, sF);
    __syncthreads();                                          // the forward counts, for other threads' frames
    emd_pass<true>(T, e0, ld, gt, fr, sh, totR, absR, sR);
    const double sumF = block_sum_d(absF, sh);
    const double sumR = block_sum_d(absR, sh);
    const int pad = (Tmax - T) * ((totF > 0.0) - (totF < 0.0));
    __syncthreads();
    for (int t = threadIdx.x; t < Tmax; t += kScanThreads) fr[t] = t < T ? fr[t] + sF + sR + pad : 0;
    if (threadIdx.x == 0) {
        sums[3 * b] = sumF;                                   // the row's own frames only: the same bits in any batch
        sums[3 * b + 1] = sumR;
        sums[3 * b + 2] = fabs(totF);                         // each padding column's |forward sum|
    }
}

// ---- reduction: one workgroup per row, then one wave for the batch -----------------------------------------------
__global__ __launch_bounds__(256) void fa_reduce_rows_kernel(
    int B, int Tmax, int V, int nb, const int32_t* __restrict__ Tv, const int32_t* __restrict__ ltv,
    const float* __restrict__ terms, const int32_t* __restrict__ bins, const int32_t* __restrict__ ph_frame,
    const double* __restrict__ emd_sums, double* __restrict__ row_terms, int32_t* __restrict__ hist) {
    __shared__ int h[kMaxV + 3 * kMaxBins + 6];
    __shared__ double red[3][4];
    const int H = V + 3 * nb + 6;
    const int o_gd = V, o_egd = V + nb, o_elab = V + 2 * nb, o_dgd = V + 2 * nb + 3, o_dlab = V + 3 * nb + 3;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const bool full = ltv[b] >= 2;
        const int T = full ? min(max(Tv[b], 0), Tmax) : 0;
        for (int i = tid; i < H; i += 256) h[i] = 0;
        __syncthreads();
        double a[3] = {0.0, 0.0, 0.0};
        for (int t = tid; t < T; t += 256) {
            const size_t ft = (size_t)b * Tmax + t;
#pragma unroll
            for (int k = 0; k < 3; ++k) a[k] += (double)terms[ft * 3 + k];
            const int32_t* bn = bins + ft * 5;
            const int bf = bn[0], be = bn[1], le = bn[2], bd = bn[3], l2 = bn[4];
            if (bf >= 0 && bf < nb) {
                atomicAdd(&h[min(max(ph_frame[ft], 0), V - 1)], 1);
                atomicAdd(&h[o_gd + bf], 1);
            }
            if (be >= 0 && be < nb && le >= 0 && le < 3) {
                atomicAdd(&h[o_egd + be], 1);
                atomicAdd(&h[o_elab + le], 1);
            }
            if (bd >= 0 && bd < nb && l2 >= 0 && l2 < 3) {
                atomicAdd(&h[o_dgd + bd], 1);
                atomicAdd(&h[o_dlab + l2], 1);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a[k] = hfa::wave_sum_d(a[k]);
            if (lane == 0) red[k][wave] = a[k];
        }
        __syncthreads();
        if (tid == 0) {
            double r[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) r[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
            row_terms[4 * b + 0] = r[0];
            row_terms[4 * b + 1] = r[1];
            const double* es = emd_sums + 3 * b;              // the padding columns' share in closed form
            row_terms[4 * b + 2] = full ? ((es[0] + (double)(Tmax - T) * es[2]) + es[1]) * 0.5 : 0.0;
            row_terms[4 * b + 3] = r[2];
        }
        for (int i = tid; i < H; i += 256) {
            if (h[i] != 0) atomicAdd(&hist[i], h[i]);          // integer: order-free
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void fa_reduce_batch_kernel(int B, int Tmax, int V, int nb,
                                                             const int32_t* __restrict__ ltv,
                                                             const double* __restrict__ row_terms,
                                                             const int32_t* __restrict__ hist,
                                                             double* __restrict__ losses, double* __restrict__ norm) {
    const int k = threadIdx.x;
    if (k >= 4) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += row_terms[4 * b + k];    // ascending b
    long long n = 0;
    if (k == 0) {
        for (int i = 0; i < nb; ++i) n += hist[V + i];
    } else if (k == 1) {
        for (int i = 0; i < 3; ++i) n += hist[V + 2 * nb + i];
    } else if (k == 2) {
        for (int b = 0; b < B; ++b) n += ltv[b] >= 2 ? Tmax : 0;
    } else {
        for (int i = 0; i < 3; ++i) n += hist[V + 3 * nb + 3 + i];
    }
    losses[k] = n > 0 ? s / (double)n : 0.0;
    norm[k] = (double)n;
}

bool misaligned(const void* p, size_t a) { return ((uintptr_t)p % a) != 0; }

}  // namespace

extern "C" {

int hfa_fa_frame_loss(int B, int Tmax, int V, int num_bins, double label_smoothing, const int32_t* T,
                      const int32_t* label_type, const float* logits, long long ld, long long bs,
                      const int32_t* ph_frame, const float* ph_edge, const int32_t* ph_mask, const float* tables,
                      float* terms, int32_t* bins, const float* coef, const int32_t* emd_fac, float* grad,
                      long long g_ld, long long g_bs, hipStream_t stream) {
    if (B < 0 || Tmax < 0 || V <= 0 || V > kMaxV || num_bins <= 0 || num_bins > kMaxBins) {
        hfa::set_error("hfa_fa_frame_loss: bad sizes (B, Tmax >= 0, 0 < V <= %d, 0 < num_bins <= %d)", kMaxV, kMaxBins);
        return HFA_EINVAL;
    }
    if (!(label_smoothing >= 0.0 && label_smoothing <= 0.5) || ld < 0 || bs < 0 || g_ld < 0 || g_bs < 0) {
        hfa::set_error("hfa_fa_frame_loss: bad layout (0 <= label_smoothing <= 0.5, strides >= 0)");
        return HFA_EINVAL;
    }
    if (B == 0 || Tmax == 0) return HFA_OK;
    if (!T || !label_type || !logits || !ph_frame || !ph_edge || !ph_mask || !tables || !terms || !bins ||
        (grad && !coef)) {
        hfa::set_error("hfa_fa_frame_loss: null pointer (coef is required with grad)");
        return HFA_EINVAL;
    }
    if (misaligned(T, 4) || misaligned(label_type, 4) || misaligned(logits, 4) || misaligned(ph_frame, 4) ||
        misaligned(ph_edge, 4) || misaligned(ph_mask, 4) || misaligned(tables, 4) || misaligned(terms, 4) ||
        misaligned(bins, 4) || misaligned(coef, 4) || misaligned(emd_fac, 4) || misaligned(grad, 4)) {
        hfa::set_error("hfa_fa_frame_loss: misaligned pointer (4-byte elements)");
        return HFA_EINVAL;
    }
    const int tb = (Tmax + kRowThreads / 64 - 1) / (kRowThreads / 64);
    const int gx = hfa::capped((long long)tb * B) / B;
    dim3 grid(gx > 0 ? gx : 1, B);
    hipLaunchKernelGGL(fa_frame_kernel, grid, dim3(kRowThreads), 0, stream, Tmax, V, num_bins, (float)label_smoothing,
                       (float)(1.0 - label_smoothing), T,
                       label_type, logits, ld, bs, ph_frame, ph_edge, ph_mask, tables, terms, bins, coef, emd_fac, grad,
                       g_ld, g_bs);
    return hfa::check_launch("hfa_fa_frame_loss");
}

int hfa_fa_emd(int B, int Tmax, const int32_t* T, const int32_t* label_type, const float* logits, long long ld,
               long long bs, const float* ph_edge, double* sums, int32_t* fac, hipStream_t stream) {
    if (B < 0 || Tmax < 0 || ld < 0 || bs < 0) {
        hfa::set_error("hfa_fa_emd: bad sizes (B, Tmax >= 0, strides >= 0)");
        return HFA_EINVAL;
    }
    if (B == 0) return HFA_OK;
    if (!T || !label_type || !sums || (Tmax > 0 && (!logits || !ph_edge || !fac))) {
        hfa::set_error("hfa_fa_emd: null pointer");
        return HFA_EINVAL;
    }
    if (misaligned(T, 4) || misaligned(label_type, 4) || misaligned(logits, 4) || misaligned(ph_edge, 4) ||
        misaligned(sums, 8) || misaligned(fac, 4)) {
        hfa::set_error("hfa_fa_emd: misaligned pointer (4-byte elements, sums 8)");
        return HFA_EINVAL;
    }
    hipLaunchKernelGGL(fa_emd_kernel, dim3(B), dim3(kScanThreads), 0, stream, Tmax, T, label_type, logits, ld, bs,
                       ph_edge, sums, fac);
    return hfa::check_launch("hfa_fa_emd");
}

int hfa_fa_loss_reduce(int B, int Tmax, int V, int num_bins, const int32_t* T, const int32_t* label_type,
                       const float* terms, const int32_t* bins, const int32_t* ph_frame, const double* emd_sums,
                       double* row_terms, double* losses, double* norm, int32_t* hist, hipStream_t stream) {
    if (B < 0 || Tmax < 0 || V <= 0 || V > kMaxV || num_bins <= 0 || num_bins > kMaxBins) {
        hfa::set_error("hfa_fa_loss_reduce: bad sizes (B, Tmax >= 0, 0 < V <= %d, 0 < num_bins <= %d)", kMaxV,
                       kMaxBins);
        return HFA_EINVAL;
    }
    if (!losses || !norm || !hist || (B > 0 && (!T || !label_type || !emd_sums || !row_terms)) ||
        (B > 0 && Tmax > 0 && (!terms || !bins || !ph_frame))) {
        hfa::set_error("hfa_fa_loss_reduce: null pointer");
        return HFA_EINVAL;
    }
    if (misaligned(T, 4) || misaligned(label_type, 4) || misaligned(terms, 4) || misaligned(bins, 4) ||
        misaligned(ph_frame, 4) || misaligned(emd_sums, 8) || misaligned(row_terms, 8) || misaligned(losses, 8) ||
        misaligned(norm, 8) || misaligned(hist, 4)) {
        hfa::set_error("hfa_fa_loss_reduce: misaligned pointer (4-byte elements, the f64 arrays 8)");
        return HFA_EINVAL;
    }
    hipError_t e = hipMemsetAsync(hist, 0, sizeof(int32_t) * (size_t)(V + 3 * num_bins + 6), stream);
    if (e != hipSuccess) {
        hfa::set_error("hfa_fa_loss_reduce: clearing hist failed: %s", hipGetErrorString(e));
        return -(int)e;
    }
    if (B > 0) {
        hipLaunchKernelGGL(fa_reduce_rows_kernel, dim3(hfa::capped(B)), dim3(256), 0, stream, B, Tmax, V, num_bins, T,
                           label_type, terms, bins, ph_frame, emd_sums, row_terms, hist);
        const int rc = hfa::check_launch("hfa_fa_loss_reduce");
        if (rc != HFA_OK) return rc;
    }
    hipLaunchKernelGGL(fa_reduce_batch_kernel, dim3(1), dim3(64), 0, stream, B, Tmax, V, num_bins, label_type,
                       row_terms, hist, losses, norm);
    return hfa::check_launch("hfa_fa_loss_reduce");
}

}  // extern "C"
