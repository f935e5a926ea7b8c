// melspec.hip — fused log-mel spectrogram (tools/get_melspec.py:28-54) on the split-f16 MFMA scheme of gemm.hip.
//
// out[b, m, f] = log(max(sum_bin |STFT(x_b)[f, bin]| fb[bin, m], clamp)): a windowed DFT, a magnitude, the mel
// filterbank and the log in ONE kernel; the spectrum never leaves the chip.  Both contractions are three-product
// split-f16 (x1 = f16(x), x2 = f16((x - x1) 2^11), A.W = A1.W1 + 2^-11 (A1.W2 + A2.W1), f32 accumulation in a
// single accumulator that carries 2^11 x the sum) on v_mfma_f32_16x16x32_f16.
//
// A workgroup (4 waves) owns FT = 16 RB frames of one row:
//   - it stages the samples those frames read once, split on load into two f16 planes in LDS and masked against the
//     row's own length (samples outside [0, lens[b]) are zeros whatever the caller's buffer holds).  Frame f, tap k is
//     LDS sample f * min(hop, win) + k, so overlapping frames share their samples; 16 B of padding every
//     2^padshift samples keep the 16 frame rows of an operand read on different banks;
//   - it walks the needed bins in chunks of 64: wave w accumulates frames x (16 cos + 16 sin columns) of bins
//     16 w .. 16 w + 15 of the chunk over K = win (padded to 128 with zero basis columns).  The basis streams from
//     global memory straight into registers in MFMA fragment order (1 KiB per wave load, nothing shared between
//     waves), four K-steps ahead of the MFMAs;
//   - re and im of one bin land in the same lane and register, so the magnitude is lane-local; it is split and
//     written to a [frame][64 bins] LDS image, and the second contraction (mel rows x frames, K = 64 bins) adds the
//     chunk into a resident 128 x FT accumulator (wave w: mels 32 w .. 32 w + 31);
//   - after the last chunk it writes log(max(acc, clamp)) for the row's own frames and zeros past them.
// Every output element sums the same products in the same order whatever FT, the batch or the row's position.
#include "hfa_common.h"
#include "hfa.h"

#include <math.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kMagLd = 72;          // halves per frame row of the magnitude image (64 bins + 16 B: conflict-free reads)
constexpr int kMelPad = 128;        // mel rows of the filterbank table (n_mels <= 128, zero rows past n_mels)
constexpr int kLdsBytes = 160 * 1024;

struct MelP {
    int N, win, Kpad, hop, lstride, padshift, n_mels, nchunks, frames, a_halves;
    const float* x;
    long long x_bs;
    const int32_t* lens;
    const _Float16* basis;      // [2][nchunks * 8 column blocks][Kpad / 32][64 lanes][8]
    long long sBp;
    const _Float16* fb;         // [2][8 mel blocks][nchunks * 2][64 lanes][8]
    long long sFp;
    float clamp, log_clamp;
    float* y;
    long long y_bs;
    int y_ld;
    int* oflow;
};

template <int RB>
__global__ __launch_bounds__(256) void logmel_split_kernel(const MelP p) {
    constexpr int FT = RB * 16;
    extern __shared__ __attribute__((aligned(16))) _Float16 smem[];
    _Float16* sA1 = smem;
    _Float16* sA2 = smem + p.a_halves;
    _Float16* sM1 = smem + 2 * p.a_halves;
    _Float16* sM2 = sM1 + FT * kMagLd;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, q = lane >> 4;
    const int b = blockIdx.y, f0 = blockIdx.x * FT;
    int len = p.lens ? p.lens[b] : p.N;
    len = len < 0 ? 0 : (len > p.N ? p.N : len);
    const int nf = len / p.hop + 1;
    float* yb = p.y + (long long)b * p.y_bs;

    if (f0 >= nf) {                                  // a tile past the row's frames: zeros
        for (int i = tid; i < p.n_mels * FT; i += 256) {
            const int m = i / FT, f = f0 + (i - m * FT);
            if (f < p.frames) yb[(long long)m * p.y_ld + f] = 0.0f;
        }
        return;
    }

    // ---- stage the tile's samples as split planes (masked against [0, len)) ----
    {
        const float* xr = p.x + (long long)b * p.x_bs;
        const int total = (FT - 1) * p.lstride + p.Kpad;
        const int half = p.win / 2;
        for (int i = tid * 8; i < total; i += 256 * 8) {
            int f = i / p.lstride;
            f = f < FT - 1 ? f : FT - 1;
            const int k = i - f * p.lstride;
            const long long g = (long long)(f0 + f) * p.hop - half + k;
            float v[8];
            if (g >= 0 && g + 8 <= len) {
                const f32x4 lo = *reinterpret_cast<const f32x4*>(xr + g);
                const f32x4 hi = *reinterpret_cast<const f32x4*>(xr + g + 4);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    v[t] = lo[t];
                    v[4 + t] = hi[t];
                }
            } else {
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const long long s = g + t;
                    v[t] = (s >= 0 && s < len) ? xr[s] : 0.0f;
                }
            }
            f16x8 h, l;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                h[t] = (_Float16)v[t];
                l[t] = (_Float16)((v[t] - (float)h[t]) * 2048.0f);
            }
            const int phys = i + ((i >> p.padshift) << 3);
            *reinterpret_cast<f16x8*>(sA1 + phys) = h;
            *reinterpret_cast<f16x8*>(sA2 + phys) = l;
        }
    }
    __syncthreads();

    int rowbase[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) rowbase[i] = (i * 16 + r16) * p.lstride + 8 * q;

    f32x4 acc[RB][2], acc2[2][RB];
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            acc2[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }

    const int nks = p.Kpad / 32, gpc = p.Kpad / 128, G = p.nchunks * gpc;
    const _Float16* bl = p.basis + lane * 8;
    const _Float16* fl = p.fb + lane * 8;
    bool bad = false;

    f16x8 bufA[4][2][2], bufB[4][2][2], fbf[2][2][2];      // [K-step][cos, sin][plane]; [K-step][mel block][plane]
    auto load_basis = [&](f16x8 (&buf)[4][2][2], int g) {
        const int c = g / gpc, kg = g - c * gpc;
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            const long long cb = c * 8 + wave * 2 + part;
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    buf[s][part][pl] =
                        *reinterpret_cast<const f16x8*>(bl + pl * p.sBp + (cb * nks + kg * 4 + s) * 512);
        }
    };
    auto compute = [&](const f16x8 (&buf)[4][2][2], int kg) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k0 = kg * 128 + s * 32;
            f16x8 a1[RB], a2[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                const int idx = rowbase[i] + k0;
                const int phys = idx + ((idx >> p.padshift) << 3);
                a1[i] = *reinterpret_cast<const f16x8*>(sA1 + phys);
                a2[i] = *reinterpret_cast<const f16x8*>(sA2 + phys);
            }
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                const f16x8 w1 = buf[s][part][0], w2 = buf[s][part][1];
                const f16x8 w1s = w1 * (_Float16)2048.0f;
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    acc[i][part] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[i], w1s, acc[i][part], 0, 0, 0);
                    acc[i][part] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[i], w2, acc[i][part], 0, 0, 0);
                    acc[i][part] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[i], w1, acc[i][part], 0, 0, 0);
                }
            }
        }
    };
    // end of a bin chunk: magnitudes -> split planes in LDS -> mel accumulator += fb rows x magnitudes
    auto chunk_end = [&]() {
        __syncthreads();                             // the previous chunk's magnitude reads are done
#pragma unroll
        for (int i = 0; i < RB; ++i) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float re = acc[i][0][e] * (1.0f / 2048.0f), im = acc[i][1][e] * (1.0f / 2048.0f);
                const float mag = sqrtf(re * re + im * im);
                const int fr = i * 16 + 4 * q + e;
                bad |= !(mag < 65504.0f) && f0 + fr < nf;
                const _Float16 m1 = (_Float16)mag;
                sM1[fr * kMagLd + wave * 16 + r16] = m1;
                sM2[fr * kMagLd + wave * 16 + r16] = (_Float16)((mag - (float)m1) * 2048.0f);
            }
            acc[i][0] = f32x4{0.f, 0.f, 0.f, 0.f};
            acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            f16x8 m1[RB], m2[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                const int o = (i * 16 + r16) * kMagLd + ks * 32 + 8 * q;
                m1[i] = *reinterpret_cast<const f16x8*>(sM1 + o);
                m2[i] = *reinterpret_cast<const f16x8*>(sM2 + o);
            }
#pragma unroll
            for (int jm = 0; jm < 2; ++jm) {
                const f16x8 w1 = fbf[ks][jm][0], w2 = fbf[ks][jm][1];
                const f16x8 w1s = w1 * (_Float16)2048.0f;
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    acc2[jm][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1s, m1[i], acc2[jm][i], 0, 0, 0);
                    acc2[jm][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w2, m1[i], acc2[jm][i], 0, 0, 0);
                    acc2[jm][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1, m2[i], acc2[jm][i], 0, 0, 0);
                }
            }
        }
    };
    auto step = [&](const f16x8 (&cur)[4][2][2], f16x8 (&nxt)[4][2][2], int g) {
        const int c = g / gpc, kg = g - c * gpc;
        const bool last = kg == gpc - 1;
        if (g + 1 < G) load_basis(nxt, g + 1);
        if (last) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int jm = 0; jm < 2; ++jm)
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl)
                        fbf[ks][jm][pl] = *reinterpret_cast<const f16x8*>(
                            fl + pl * p.sFp + ((long long)(wave * 2 + jm) * (p.nchunks * 2) + c * 2 + ks) * 512);
        }
        compute(cur, kg);
        if (last) chunk_end();
    };

    load_basis(bufA, 0);
    for (int g = 0; g < G; g += 2) {
        step(bufA, bufB, g);
        if (g + 1 < G) step(bufB, bufA, g + 1);
    }

    // ---- log(max(mel, clamp)): accumulator rows are mels (4 q + e), columns frames (lane & 15) ----
#pragma unroll
    for (int jm = 0; jm < 2; ++jm)
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int f = f0 + i * 16 + r16;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int m = wave * 32 + jm * 16 + 4 * q + e;
                const float v = acc2[jm][i][e] * (1.0f / 2048.0f);
                const float o = v <= p.clamp ? p.log_clamp : logf(v);
                if (m < p.n_mels && f < p.frames) yb[(long long)m * p.y_ld + f] = f < nf ? o : 0.0f;
            }
        }
    if (bad && p.oflow) *p.oflow = 1;
}

inline bool al16(const void* ptr) { return ((uintptr_t)ptr & 15) == 0; }

template <int RB>
int launch(const MelP& p, int B, size_t lds, hipStream_t stream) {
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute((const void*)logmel_split_kernel<RB>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            hfa::set_error("hfa_logmel_split: cannot reserve %zu B of LDS: %s", lds, hipGetErrorString(e));
            return -(int)e;
        }
    }
    constexpr int FT = RB * 16;
    hipLaunchKernelGGL(logmel_split_kernel<RB>, dim3((p.frames + FT - 1) / FT, B), dim3(256), lds, stream, p);
    return hfa::check_launch("hfa_logmel_split");
}

}  // namespace

extern "C" {

int hfa_logmel_split(int B, int N, const float* x, long long x_bs, const int32_t* lens, int win_length, int hop,
                     int n_fft, int n_mels, int nb_pad, const uint16_t* basis, const uint16_t* fb, float clamp,
                     int frames, float* y, long long y_bs, int y_ld, int* oflow, hipStream_t stream) {
    if (B < 0 || N < 1 || frames < 1 || win_length < 32 || win_length > 2048 || win_length % 32 || n_fft % 2 ||
        n_fft < win_length || hop < 8 || hop % 8 || n_mels < 1 || n_mels > kMelPad || nb_pad < 64 || nb_pad % 64 ||
        nb_pad > n_fft / 2 + 64 || !(clamp >= 0.0f) || x_bs % 4 || y_ld < frames) {
        hfa::set_error("hfa_logmel_split: outside the supported envelope (win_length a multiple of 32 and <= 2048, "
                       "n_fft even and >= win_length, hop a multiple of 8, n_mels <= 128, nb_pad a multiple of 64, "
                       "x_bs a multiple of 4, y_ld >= frames)");
        return HFA_EINVAL;
    }
    if (!x || !basis || !fb || !y || !al16(x) || !al16(basis) || !al16(fb) || !al16(y)) {
        hfa::set_error("hfa_logmel_split: x, basis, fb and y must be non-NULL and 16-B aligned");
        return HFA_EINVAL;
    }
    if (B == 0) return HFA_OK;
    if (B > 65535) {
        hfa::set_error("hfa_logmel_split: B <= 65535");
        return HFA_EINVAL;
    }
    MelP p;
    p.N = N;
    p.win = win_length;
    p.Kpad = (win_length + 127) / 128 * 128;
    p.hop = hop;
    p.lstride = hop < win_length ? hop : win_length;
    p.padshift = 31 - __builtin_clz((unsigned)p.lstride);
    p.n_mels = n_mels;
    p.nchunks = nb_pad / 64;
    p.frames = frames;
    p.x = x;
    p.x_bs = x_bs;
    p.lens = lens;
    p.basis = reinterpret_cast<const _Float16*>(basis);
    p.sBp = (long long)p.nchunks * 8 * (p.Kpad / 32) * 512;
    p.fb = reinterpret_cast<const _Float16*>(fb);
    p.sFp = (long long)8 * p.nchunks * 2 * 512;
    p.clamp = clamp;
    p.log_clamp = (float)log((double)clamp);
    p.y = y;
    p.y_bs = y_bs;
    p.y_ld = y_ld;
    p.oflow = oflow;
    // the largest frame tile whose sample window fits the LDS (results do not depend on it)
    for (int rb = 4; rb >= 1; rb >>= 1) {
        const int FT = rb * 16;
        const int total = (FT - 1) * p.lstride + p.Kpad;
        p.a_halves = total + ((total >> p.padshift) << 3) + 8;
        const size_t lds = ((size_t)2 * p.a_halves + (size_t)2 * FT * kMagLd) * 2;
        if (lds > (size_t)kLdsBytes) continue;
        return rb == 4 ? launch<4>(p, B, lds, stream) : rb == 2 ? launch<2>(p, B, lds, stream)
                                                                : launch<1>(p, B, lds, stream);
    }
    hfa::set_error("hfa_logmel_split: no frame tile fits the LDS");
    return HFA_EINVAL;
}

}  // extern "C"
