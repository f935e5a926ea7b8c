// train.hip — the two kernels head fine-tuning needs beyond the losses' d loss / d logits:
//   * hfa_wgrad_f32: the weight gradient of an nn.Linear over a variable-length batch (what autograd's addmm backward
//     gives the head of networks/task/forced_alignment.py:53-55), dW = G^T X and db = column sums of G over the rows
//     t < lens[b], plus the squared norm of both for the clip;
//   * hfa_adamw_f32: torch.nn.utils.clip_grad_norm_ (train.py:139-141's gradient_clip_val) and one torch.optim.AdamW
//     step (forced_alignment.py:473-486) over a flat parameter buffer, in one launch.
//
// The weight gradient's output is tiny (65 x 192) and its reduction long (27 552 rows at config 2), so the
// parallelism is a split of the reduction: chunk q = (b, t / kChunk) covers rows t of batch row b only, whatever the
// grid, and writes its f32 partial of dW (a k-ordered v_mfma_f32_16x16x4_f32 chain, bit for bit an fmaf chain over
// the rows in ascending t) and its f64 partial of db (column sums need no product: plain f64 adds, so a bias gradient
// that nearly cancels keeps its digits) into the workspace; a second pass adds the live chunks' partials in ascending q in f64, and a
// third adds the squares of what the second wrote, block by block in ascending order.  No float atomics, no
// arrival order: the same bits on every run and under any grid cap.
#include "hfa_common.h"
#include "hfa.h"

#include <math.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kChunk = 256;      // rows of one batch row per partial (a multiple of 16: the unrolled k-steps)
constexpr int kNT = 5;           // 16-row tiles of dW per pass over the chunk: N <= 80 (the workload's 65) in one pass
constexpr int kCT = 2;           // 16-column tiles of dW per wave
constexpr int kWaves = 4;
constexpr int kUnroll = 4;      // k-steps (of 4 rows) whose loads are in flight together
constexpr int kSumBlock = 256;   // outputs per squared-norm partial

// the workspace: [nsum] f64 squared-norm partials, per chunk an [N] f64 partial of db, per chunk an [N][C] f32 partial
// of dW
__host__ __device__ inline long long n_sum_blocks(long long n_out) { return (n_out + kSumBlock - 1) / kSumBlock; }

__global__ __launch_bounds__(kWaves * 64) void wgrad_chunk_kernel(
    int n_chunks, int nct, int Tmax, int N, int C, const float* __restrict__ G, long long ldg, long long g_bs,
    const float* __restrict__ X, long long ldx, long long x_bs, const int32_t* __restrict__ lens,
    float* __restrict__ part, double* __restrict__ part_db) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int c0 = (blockIdx.y * kWaves + wave) * (16 * kCT);
    if (c0 >= C) return;                                   // (no barrier below: a wave may leave alone)
    const int lc = lane & 15, lk = lane >> 4;
    const long long rec = (long long)N * C;
    for (int q = blockIdx.x; q < n_chunks; q += gridDim.x) {
        const int b = q / nct;
        const int t0 = (q - b * nct) * kChunk;
        int len = lens[b];
        len = len < 0 ? 0 : (len > Tmax ? Tmax : len);
        if (t0 >= len) continue;                           // a chunk of padding: the second pass skips it too
        const int rows = len - t0 < kChunk ? len - t0 : kChunk;
        const float* Gb = G + (long long)b * g_bs;
        const float* Xb = X + (long long)b * x_bs;
        float* P = part + (long long)q * rec;
        for (int n0 = 0; n0 < N; n0 += 16 * kNT) {
            f32x4 acc[kNT][kCT];
            double accb[kNT];                              // db: each lane's own rows in f64 (exact to the last bit or two)
#pragma unroll
            for (int i = 0; i < kNT; ++i) {
                accb[i] = 0.0;
#pragma unroll
                for (int j = 0; j < kCT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            for (int r = 0; r < rows; r += 4 * kUnroll) {
                // lane (lc, lk): A[n = lc][k = lk] = G[t, n0 + 16 i + lc], B[k = lk][c = lc] = X[t, c0 + 16 j + lc],
                // t = t0 + r + 4 u + lk; a row past the length, a column past N or C is a zero that is never loaded.
                // kUnroll k-steps' loads are issued before the first MFMA, in the order the chain consumes them
                float a[kUnroll][kNT], x[kUnroll][kCT];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const int t = t0 + r + 4 * u + lk;
                    const bool live = t < len;
#pragma unroll
                    for (int i = 0; i < kNT; ++i) {
                        const int n = n0 + 16 * i + lc;
                        a[u][i] = live && n < N ? Gb[(long long)t * ldg + n] : 0.f;
                    }
#pragma unroll
                    for (int j = 0; j < kCT; ++j) {
                        const int c = c0 + 16 * j + lc;
                        x[u][j] = live && c < C ? Xb[(long long)t * ldx + c] : 0.f;
                    }
                }
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
                    for (int i = 0; i < kNT; ++i) {
#pragma unroll
                        for (int j = 0; j < kCT; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][i], x[u][j], acc[i][j], 0, 0, 0);
                    }
                    if (c0 == 0) {
#pragma unroll
                        for (int i = 0; i < kNT; ++i) accb[i] += (double)a[u][i];
                    }
                }
            }
            // D: column lane & 15 (c), row 4 (lane >> 4) + e (n)
#pragma unroll
            for (int i = 0; i < kNT; ++i) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int n = n0 + 16 * i + 4 * lk + e;
                    if (n >= N) continue;
#pragma unroll
                    for (int j = 0; j < kCT; ++j) {
                        const int c = c0 + 16 * j + lc;
                        if (c < C) P[(long long)n * C + c] = acc[i][j][e];
                    }
                }
            }
            if (c0 == 0) {                                 // the four row groups of a column, in a fixed order
#pragma unroll
                for (int i = 0; i < kNT; ++i) {
                    double s = accb[i];
                    s += __shfl_xor(s, 16, 64);
                    s += __shfl_xor(s, 32, 64);
                    const int n = n0 + 16 * i + lc;
                    if (lk == 0 && n < N) part_db[(long long)q * N + n] = s;
                }
            }
        }
    }
}

// output o < N C: dW[o / C][o % C]; N C <= o < N C + N: db[o - N C].  Partials of the live chunks in ascending q, f64.
__global__ __launch_bounds__(kSumBlock) void wgrad_sum_kernel(int n_chunks, int nct, int Tmax, int N, int C,
                                                              const int32_t* __restrict__ lens,
                                                              const float* __restrict__ part,
                                                              const double* __restrict__ part_db,
                                                              float* __restrict__ dW,
                                                              long long ldw, float* __restrict__ db,
                                                              double* __restrict__ sq) {
    __shared__ double red[kSumBlock / 64];
    const long long nc = (long long)N * C, n_out = nc + N;
    const long long blocks = n_sum_blocks(n_out);
    for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
        const long long o = blk * kSumBlock + threadIdx.x;
        double s2 = 0.0;
        if (o < n_out) {
            double s = 0.0;
            for (int q = 0; q < n_chunks; ++q) {
                const int b = q / nct;
                const int len = lens[b] > Tmax ? Tmax : lens[b];
                if ((q - b * nct) * kChunk < len)
                    s += o < nc ? (double)part[(long long)q * nc + o] : part_db[(long long)q * N + (o - nc)];
            }
            const float r = (float)s;
            if (o < nc) dW[(o / C) * ldw + o % C] = r;
            else db[o - nc] = r;
            s2 = (double)r * (double)r;
        }
        s2 = hfa::wave_sum_d(s2);                          // a fixed tree over the block's 256 outputs
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s2;
        __syncthreads();
        if (threadIdx.x == 0) sq[blk] = (red[0] + red[1]) + (red[2] + red[3]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void wgrad_norm_kernel(long long blocks, const double* __restrict__ sq,
                                                        double* __restrict__ sumsq) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (long long i = 0; i < blocks; ++i) s += sq[i];     // ascending
    *sumsq = s;
}

__global__ __launch_bounds__(256) void adamw_kernel(long long n, float* __restrict__ p, float* __restrict__ m,
                                                    float* __restrict__ v, const float* __restrict__ g,
                                                    const double* __restrict__ sumsq, double max_norm, double decay,
                                                    double beta1, double beta2, double eps, double step_size,
                                                    double inv_sqrt_bc2, int32_t* __restrict__ skipped) {
    const double ss = *sumsq;
    if (!(fabs(ss) <= 1.79769313486231570815e308)) {       // inf or NaN: the step is skipped, nothing is written
        if (blockIdx.x == 0 && threadIdx.x == 0) *skipped += 1;      // (launches are stream-ordered: one writer)
        return;
    }
    // clip_grad_norm_: the gradient times min(1, max_norm / (norm + 1e-6)), as an f32 factor on f32 gradients
    float coef = 1.0f;
    if (max_norm > 0.0) {
        const double c = max_norm / (sqrt(ss) + 1e-6);
        coef = (float)(c < 1.0 ? c : 1.0);
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double gi = (double)(g[i] * coef);
        const double pi = (double)p[i] * decay;
        const double mi = beta1 * (double)m[i] + (1.0 - beta1) * gi;
        const double vi = beta2 * (double)v[i] + (1.0 - beta2) * gi * gi;
        const float mf = (float)mi, vf = (float)vi;        // the state the next step reads
        m[i] = mf;
        v[i] = vf;
        p[i] = (float)(pi - step_size * (double)mf / (sqrt((double)vf) * inv_sqrt_bc2 + eps));
    }
}

bool misaligned(const void* p, size_t a) { return ((uintptr_t)p % a) != 0; }

// the shape checks hfa_wgrad_f32 and hfa_wgrad_workspace_bytes share; the number of chunks or -1
long long wgrad_chunks(int B, int Tmax, int N, int C) {
    if (B < 0 || Tmax < 0 || N < 1 || C < 8 || C % 8 != 0) return -1;
    const long long nct = ((long long)Tmax + kChunk - 1) / kChunk;
    const long long chunks = nct * B, n_out = (long long)N * C + N;
    if (chunks > 0x7fffffffLL || n_out > 0x7fffffffLL) return -1;
    return chunks;
}

}  // namespace

extern "C" {

long long hfa_wgrad_workspace_bytes(int B, int Tmax, int N, int C) {
    const long long chunks = wgrad_chunks(B, Tmax, N, C);
    if (chunks < 0) {
        hfa::set_error("hfa_wgrad_workspace_bytes: bad sizes (B, Tmax >= 0, N >= 1, C a positive multiple of 8)");
        return HFA_EINVAL;
    }
    const long long n_out = (long long)N * C + N;
    return 8 * n_sum_blocks(n_out) + 8 * chunks * N + 4 * chunks * N * C;
}

int hfa_wgrad_f32(int B, int Tmax, int N, int C, const float* G, long long ldg, long long g_bs, const float* X,
                  long long ldx, long long x_bs, const int32_t* lens, float* dW, long long ldw, float* db,
                  double* sumsq, void* workspace, hipStream_t stream) {
    const long long chunks = wgrad_chunks(B, Tmax, N, C);
    if (chunks < 0) {
        hfa::set_error("hfa_wgrad_f32: bad sizes (B, Tmax >= 0, N >= 1, C a positive multiple of 8)");
        return HFA_EINVAL;
    }
    if (ldg < N || ldx < C || ldw < C || g_bs < 0 || x_bs < 0) {
        hfa::set_error("hfa_wgrad_f32: bad layout (ldg >= N, ldx >= C, ldw >= C, batch strides >= 0)");
        return HFA_EINVAL;
    }
    if (!dW || !db || !sumsq || !workspace || (B > 0 && !lens) || (chunks > 0 && (!G || !X))) {
        hfa::set_error("hfa_wgrad_f32: null pointer");
        return HFA_EINVAL;
    }
    if (misaligned(G, 4) || misaligned(X, 4) || misaligned(lens, 4) || misaligned(dW, 4) || misaligned(db, 4) ||
        misaligned(sumsq, 8) || misaligned(workspace, 8)) {
        hfa::set_error("hfa_wgrad_f32: misaligned pointer (4-byte elements; sumsq and the workspace 8)");
        return HFA_EINVAL;
    }
    const long long n_out = (long long)N * C + N;
    const long long blocks = n_sum_blocks(n_out);
    double* sq = (double*)workspace;
    double* part_db = sq + blocks;
    float* part = (float*)(part_db + chunks * N);
    const int nct = (Tmax + kChunk - 1) / kChunk;
    if (chunks > 0) {
        dim3 grid(hfa::capped(chunks), (C + 16 * kCT * kWaves - 1) / (16 * kCT * kWaves));
        hipLaunchKernelGGL(wgrad_chunk_kernel, grid, dim3(kWaves * 64), 0, stream, (int)chunks, nct, Tmax, N, C, G, ldg,
                           g_bs, X, ldx, x_bs, lens, part, part_db);
        const int rc = hfa::check_launch("hfa_wgrad_f32");
        if (rc != HFA_OK) return rc;
    }
    hipLaunchKernelGGL(wgrad_sum_kernel, dim3(hfa::capped(blocks)), dim3(kSumBlock), 0, stream, (int)chunks, nct, Tmax,
                       N, C, lens, part, part_db, dW, ldw, db, sq);
    int rc = hfa::check_launch("hfa_wgrad_f32");
    if (rc != HFA_OK) return rc;
    hipLaunchKernelGGL(wgrad_norm_kernel, dim3(1), dim3(64), 0, stream, blocks, sq, sumsq);
    return hfa::check_launch("hfa_wgrad_f32");
}

int hfa_wgrad_chunk_rows(void) { return kChunk; }

int hfa_adamw_f32(long long n, float* p, float* m, float* v, const float* g, const double* sumsq, double max_norm,
                  double lr, double beta1, double beta2, double eps, double weight_decay, double bc1, double bc2,
                  int32_t* skipped, hipStream_t stream) {
    if (n < 0) {
        hfa::set_error("hfa_adamw_f32: bad size (n >= 0)");
        return HFA_EINVAL;
    }
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) ||
        !(weight_decay >= 0.0) || !(bc1 > 0.0) || !(bc2 > 0.0) || max_norm != max_norm) {
        hfa::set_error("hfa_adamw_f32: bad hyper-parameter (lr, eps, weight_decay >= 0, 0 <= beta < 1, bc1, bc2 > 0)");
        return HFA_EINVAL;
    }
    if (!p || !m || !v || !g || !sumsq || !skipped) {
        hfa::set_error("hfa_adamw_f32: null pointer");
        return HFA_EINVAL;
    }
    if (misaligned(p, 4) || misaligned(m, 4) || misaligned(v, 4) || misaligned(g, 4) || misaligned(sumsq, 8) ||
        misaligned(skipped, 4)) {
        hfa::set_error("hfa_adamw_f32: misaligned pointer (4-byte elements, sumsq 8)");
        return HFA_EINVAL;
    }
    if (n == 0) return HFA_OK;
    long long blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, n, p, m, v, g, sumsq, max_norm,
                       1.0 - lr * weight_decay, beta1, beta2, eps, lr / bc1, 1.0 / sqrt(bc2), skipped);
    return hfa::check_launch("hfa_adamw_f32");
}

}  // extern "C"
