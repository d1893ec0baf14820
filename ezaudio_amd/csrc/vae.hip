// Oobleck VAE decoder building blocks (reference:
// src/modules/stable_vae/models/autoencoders.py:38-61,82-113,149-190, models/blocks.py:317-358, nn/layers.py:9-14).
//
// Every Conv1d / ConvTranspose1d of the decoder is run on the SAME bf16 MFMA GEMM as the DiT projections:
//   * activations are kept token-major [L][C] (C = GEMM K), bf16, with zero "halo" rows before and after the sequence, so a
//     k-tap (dilated) convolution is one GEMM whose K dimension is taps x C: K tile t reads the activation rows shifted by
//     tap(t) * dilation rows (GemmArgs.conv_*), weights are pre-arranged [Cout][tap][Cin];
//   * ConvTranspose1d(kernel 2s, stride s, padding ceil(s/2)) is one GEMM with K = 2 Cin (x[q], x[q-1]) and N = s * Cout: the
//     output [q][r * Cout + co] IS the up-sampled sequence [(q s + r)][co], read back with a row offset of `padding`;
//   * SnakeBeta (x + sin^2(alpha x) / beta, log-scale parameters) is fused with the fp32 -> bf16 cast that feeds the next conv;
//   * residual adds ride in the GEMM epilogue (fp32).
// The layer sequence itself is host code (ezaudio_amd/vae.py): it runs once per call, not per denoising step.
#include "../../include/ezdit.h"
#include "common.h"
#include <cstring>

namespace {

__global__ __launch_bounds__(256) void k_snake_bf16(const float* __restrict__ x, int ldx, const float* __restrict__ alpha,
                                                    const float* __restrict__ inv_beta, bf16_t* __restrict__ out, int ldo,
                                                    long L, int C) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // one thread per 4 channels
    const int c4n = C >> 2;
    if (idx >= L * c4n) return;
    const long l = idx / c4n;
    const int c = (int)(idx % c4n) * 4;
    const float4 v = *reinterpret_cast<const float4*>(x + l * ldx + c);
    float r[4] = {v.x, v.y, v.z, v.w};
    if (alpha) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float s = sinf(r[e] * alpha[c + e]);
            r[e] = r[e] + inv_beta[c + e] * s * s;   // blocks.py:317-318 snake_beta
        }
    }
    uint2 o;
    o.x = pack_bf2(r[0], r[1]);
    o.y = pack_bf2(r[2], r[3]);
    *reinterpret_cast<uint2*>(out + l * ldo + c) = o;
}

// final WNConv1d(C -> 1, k = 7, padding 3, no bias) on a haloed bf16 sequence (3 zero rows each side): one wave per 64 outputs
__global__ __launch_bounds__(256) void k_conv_out1(const bf16_t* __restrict__ xb /* row 0 = position -3 */, int ldx,
                                                   const float* __restrict__ w /* [7][C] */, float* __restrict__ out, long L, int C) {
    const long l = (long)blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    float acc = 0.f;
    for (int k = 0; k < 7; ++k) {
        const bf16_t* xr = xb + (l + k) * ldx;
        const float* wr = w + k * C;
        for (int c = 0; c < C; c += 8) {
            const uint4 v = *reinterpret_cast<const uint4*>(xr + c);
            const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc += __uint_as_float(u[e] << 16) * wr[c + 2 * e];
                acc += __uint_as_float(u[e] & 0xffff0000u) * wr[c + 2 * e + 1];
            }
        }
    }
    out[l] = acc;
}

// encoder input WNConv1d(1 -> C, k = 7, padding 3): wav fp32 [T] -> x fp32 [T][C]; w fp32 [7][C]
__global__ __launch_bounds__(256) void k_conv_in1(const float* __restrict__ wav, const float* __restrict__ w,
                                                  const float* __restrict__ bias, float* __restrict__ out, long T, int C) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int c4n = C >> 2;
    if (idx >= T * c4n) return;
    const long t = idx / c4n;
    const int c = (int)(idx % c4n) * 4;
    float4 acc = *reinterpret_cast<const float4*>(bias + c);
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const long j = t + k - 3;
        const float x = (j >= 0 && j < T) ? wav[j] : 0.f;
        const float4 wk = *reinterpret_cast<const float4*>(w + k * C + c);
        acc.x = fmaf(x, wk.x, acc.x); acc.y = fmaf(x, wk.y, acc.y); acc.z = fmaf(x, wk.z, acc.z); acc.w = fmaf(x, wk.w, acc.w);
    }
    *reinterpret_cast<float4*>(out + t * C + c) = acc;
}

// VAE bottleneck (models/bottleneck.py:67-71): enc fp32 [L][2 lat] token-major (mean | scale) + noise [lat][L] -> z [lat][L]
__global__ __launch_bounds__(256) void k_vae_sample(const float* __restrict__ enc, const float* __restrict__ noise,
                                                    float* __restrict__ z, int L, int lat) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= L * lat) return;
    const int c = idx / L, l = idx % L;
    const float mean = enc[(long)l * 2 * lat + c];
    const float sc = enc[(long)l * 2 * lat + lat + c];
    const float softplus = sc > 20.f ? sc : log1pf(expf(sc));   // torch softplus, threshold 20
    z[idx] = (noise ? noise[idx] : 0.f) * (softplus + 1e-4f) + mean;
}

// ---- segment forms: B samples stacked along the token axis, sample b on rows [b * stride, b * stride + len_b) of a level, zero rows between them.  The GEMMs run
// unchanged over the stacked rows (what they compute inside a gap lands in fp32 buffers that are only read pointwise); every kernel that writes a bf16 operand buffer or
// crosses a sample boundary is here.  len_b at a level is lens[b] * mul / div (one int32 table per call serves every level).  Padding may hold NaN: values outside an
// interior are never read, and zeros are selected, not multiplied in.
__device__ __forceinline__ long seg_len(const int* __restrict__ lens, int b, long mul, long div) { return (long)lens[b] * mul / div; }

// row r of the launch (r < rows): bf16(snake(x[b * sx + l])) with b = r / so, l = r % so when b < B and l < len_b, else ZERO -- written, not assumed
__global__ __launch_bounds__(256) void k_snake_bf16_seg(const float* __restrict__ x, int ldx, const float* __restrict__ alpha,
                                                        const float* __restrict__ inv_beta, bf16_t* __restrict__ out, int ldo, long rows, int C,
                                                        const int* __restrict__ lens, int B, long mul, long div, long sx, long so) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // one thread per 4 channels
    const int c4n = C >> 2;
    if (idx >= rows * c4n) return;
    const long r = idx / c4n;
    const int c = (int)(idx % c4n) * 4;
    const long b = r / so, l = r - b * so;
    uint2 o = make_uint2(0u, 0u);
    if (b < B && l < seg_len(lens, (int)b, mul, div)) {
        const float4 v = *reinterpret_cast<const float4*>(x + (b * sx + l) * ldx + c);
        float q[4] = {v.x, v.y, v.z, v.w};
        if (alpha) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float s = sinf(q[e] * alpha[c + e]);
                q[e] = q[e] + inv_beta[c + e] * s * s;
            }
        }
        o.x = pack_bf2(q[0], q[1]);
        o.y = pack_bf2(q[2], q[3]);
    }
    *reinterpret_cast<uint2*>(out + r * ldo + c) = o;
}

// k_conv_out1 on the stacked haloed sequence (sample b's position -3 is row b * sx): out[b][l] for l < len_b, zero up to the padded width W
__global__ __launch_bounds__(256) void k_conv_out1_seg(const bf16_t* __restrict__ xb, int ldx, const float* __restrict__ w, float* __restrict__ out,
                                                       long W, int C, const int* __restrict__ lens, int B, long mul, long div, long sx) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * W) return;
    const long b = idx / W, l = idx - b * W;
    float acc = 0.f;
    if (l < seg_len(lens, (int)b, mul, div)) {
        for (int k = 0; k < 7; ++k) {
            const bf16_t* xr = xb + (b * sx + l + k) * ldx;
            const float* wr = w + k * C;
            for (int c = 0; c < C; c += 8) {
                const uint4 v = *reinterpret_cast<const uint4*>(xr + c);
                const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc += __uint_as_float(u[e] << 16) * wr[c + 2 * e];
                    acc += __uint_as_float(u[e] & 0xffff0000u) * wr[c + 2 * e + 1];
                }
            }
        }
    }
    out[idx] = acc;
}

// k_conv_in1 on wav [B][Tmax] with sample b's own bound T_b = lens[b]: row r = b * so + t of the stacked output, zero where t >= T_b (a gap row)
__global__ __launch_bounds__(256) void k_conv_in1_seg(const float* __restrict__ wav, const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ out, long rows, int C, const int* __restrict__ lens, int B, long Tmax, long so) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int c4n = C >> 2;
    if (idx >= rows * c4n) return;
    const long r = idx / c4n;
    const int c = (int)(idx % c4n) * 4;
    const long b = r / so, t = r - b * so;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const long T = b < B ? (long)lens[b] : 0;
    if (t < T) {
        acc = *reinterpret_cast<const float4*>(bias + c);
        const float* wv = wav + b * Tmax;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const long j = t + k - 3;
            const float x = (j >= 0 && j < T) ? wv[j] : 0.f;
            const float4 wk = *reinterpret_cast<const float4*>(w + k * C + c);
            acc.x = fmaf(x, wk.x, acc.x); acc.y = fmaf(x, wk.y, acc.y); acc.z = fmaf(x, wk.z, acc.z); acc.w = fmaf(x, wk.w, acc.w);
        }
    }
    *reinterpret_cast<float4*>(out + r * C + c) = acc;
}

// k_vae_sample over B samples: enc stacked (sample b's frame l is row b * se + l), noise and z padded [B][lat][Lmax]; z is zero beyond L_b
__global__ __launch_bounds__(256) void k_vae_sample_seg(const float* __restrict__ enc, const float* __restrict__ noise, float* __restrict__ z, int Lmax,
                                                        int lat, const int* __restrict__ lens, int B, long mul, long div, long se) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long per = (long)Lmax * lat;
    if (idx >= per * B) return;
    const long b = idx / per;
    const int rem = (int)(idx - b * per);
    const int c = rem / Lmax, l = rem % Lmax;
    float v = 0.f;
    if (l < seg_len(lens, (int)b, mul, div)) {
        const float* row = enc + (b * se + l) * 2 * lat;
        const float mean = row[c];
        const float sc = row[lat + c];
        const float softplus = sc > 20.f ? sc : log1pf(expf(sc));
        v = (noise ? noise[idx] : 0.f) * (softplus + 1e-4f) + mean;
    }
    z[idx] = v;
}

int launch_status(const char* what) {   // a failed launch must surface as an error code, not as stale output
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ez_fail(EZDIT_E_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
    return EZDIT_OK;
}

}  // namespace

extern "C" {

// out fp32 [M][ldo] = A . W^T (+ bias) (+ resid); conv_cpb / conv_tap_bytes as in GemmArgs.  N multiple of 4.
// Everything that cannot be computed is refused HERE, before any HIP call (include/ezdit.h lists the rules): the tile id is the caller's, and only the
// lockstep k_gemm reads conv_cpb / conv_tap_bytes -- the ping-pong, co-resident and K-split kernels would run a plain GEMM over K * 2 bytes of each row.
int ezvae_gemm(const void* A, int lda, const void* W, int ldw, int wrows, const float* bias, const float* resid, int ldr,
               float* out, int ldo, int M, int N, int K, int conv_cpb, long conv_tap_bytes, int tile, ezdit_stream stream) {
    if (M <= 0 || N <= 0) return ez_fail(EZDIT_E_INVALID, "ezvae_gemm: M=%d and N=%d must be positive", M, N);
    if (K <= 0 || K % 64 || N % 4) return ez_fail(EZDIT_E_INVALID, "ezvae_gemm: K=%d must be a positive multiple of 64 and N=%d of 4", K, N);
    if (lda < 0 || ldw < 0 || wrows <= 0 || conv_cpb < 0)
        return ez_fail(EZDIT_E_INVALID, "ezvae_gemm: lda=%d, ldw=%d, conv_cpb=%d must not be negative and wrows=%d must be positive", lda, ldw, conv_cpb, wrows);
    const bool lockstep = tile == 6 || tile == 9 || tile == 13 || tile == 25;       // k_gemm: conv addressing, resid
    const bool pp_co = tile == 60 || tile == 61 || tile == 62 || tile == 66;         // k_gemm_pp / k_gemm_co: resid (pp_store_direct), no conv addressing
    const bool ks = tile == 70 || tile == 72 || tile == 73;                          // k_gemm_ks: neither
    if (!lockstep && !pp_co && !ks) return ez_fail(EZDIT_E_UNSUPPORTED, "ezvae_gemm: tile %d is not a GEMM configuration", tile);
    if (conv_cpb != 0 && !lockstep)
        return ez_fail(EZDIT_E_UNSUPPORTED, "ezvae_gemm: tile %d does not implement conv addressing (conv_cpb=%d); tiles 6, 9, 13, 25 do", tile, conv_cpb);
    if (resid && ks) return ez_fail(EZDIT_E_UNSUPPORTED, "ezvae_gemm: tile %d does not add a residual to an fp32 output", tile);
    if (conv_cpb != 0 && conv_tap_bytes % 16) return ez_fail(EZDIT_E_INVALID, "ezvae_gemm: conv_tap_bytes=%ld must be a multiple of 16", conv_tap_bytes);
    {   // the staging offsets of A and W are 32-bit (stage_offsets, common.h): the furthest element a launch may name stays below 2^31
        const long nkt = K / 64;
        long reach = K;
        if (conv_cpb != 0) {
            const long far_tap = (nkt - 1) / conv_cpb * (conv_tap_bytes / 2);
            reach = (far_tap > 0 ? far_tap : 0) + (nkt < conv_cpb ? nkt : (long)conv_cpb) * 64;
        }
        const long a_reach = (long)(M - 1) * lda + reach, w_reach = (long)(wrows - 1) * ldw + K;
        if (a_reach >= (1L << 31) || w_reach >= (1L << 31))
            return ez_fail(EZDIT_E_INVALID, "ezvae_gemm: operand reach A=%ld / W=%ld elements does not fit the 32-bit staging offset (< 2^31)", a_reach, w_reach);
    }
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.A = (const bf16_t*)A; g.lda = lda; g.W = (const bf16_t*)W; g.ldw = ldw; g.wrows = wrows; g.bias = bias;
    g.out = out; g.ldo = ldo; g.slab_stride = 0; g.M = M; g.N = N; g.K = K; g.splitk = 1; g.epi = EPI_F32; g.tile = tile;
    g.debug = 0; g.conv_cpb = conv_cpb; g.conv_tap_bytes = conv_tap_bytes; g.resid = resid; g.ldr = ldr; g.xcd_map = 1; g.part_bf16 = 0; g.wt = 0; memset(&g.hn, 0, sizeof g.hn);
    g.gate = nullptr; g.gate_slot_stride = 0; g.cur_step = nullptr; g.row_slot = nullptr; g.rows_per_b = 1;
    (void)hipGetLastError();
    if (launch_gemm(g, (hipStream_t)stream)) return ez_fail(EZDIT_E_UNSUPPORTED, "ezvae_gemm: tile %d / shape not supported", tile);
    return launch_status("k_gemm (vae)");
}

int ezvae_snake_bf16(const float* x, int ldx, const float* alpha, const float* inv_beta, void* out, int ldo, long L, int C,
                     ezdit_stream stream) {
    if (L <= 0 || C <= 0 || C % 4) return ez_fail(EZDIT_E_INVALID, "ezvae_snake_bf16: L=%ld must be positive and C=%d a positive multiple of 4", L, C);
    const long total = L * (C / 4);
    hipLaunchKernelGGL(k_snake_bf16, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, alpha, inv_beta,
                       (bf16_t*)out, ldo, L, C);
    return launch_status("k_snake_bf16");
}

int ezvae_conv_out1(const void* xb, int ldx, const float* w, float* out, long L, int C, ezdit_stream stream) {
    if (L <= 0 || C <= 0 || C % 8) return ez_fail(EZDIT_E_INVALID, "ezvae_conv_out1: L=%ld must be positive and C=%d a positive multiple of 8", L, C);
    hipLaunchKernelGGL(k_conv_out1, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)xb, ldx, w, out, L, C);
    return launch_status("k_conv_out1");
}

int ezvae_conv_in1(const float* wav, const float* w, const float* bias, float* out, long T, int C, ezdit_stream stream) {
    if (T <= 0 || C <= 0 || C % 4) return ez_fail(EZDIT_E_INVALID, "ezvae_conv_in1: T=%ld must be positive and C=%d a positive multiple of 4", T, C);
    const long total = T * (C / 4);
    hipLaunchKernelGGL(k_conv_in1, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, wav, w, bias, out, T, C);
    return launch_status("k_conv_in1");
}

int ezvae_sample(const float* enc, const float* noise, float* z, int L, int latent_dim, ezdit_stream stream) {
    if (L <= 0 || latent_dim <= 0 || (long)L * latent_dim >= (1L << 31))
        return ez_fail(EZDIT_E_INVALID, "ezvae_sample: L=%d and latent_dim=%d must be positive, with L * latent_dim < 2^31", L, latent_dim);
    const int total = L * latent_dim;
    hipLaunchKernelGGL(k_vae_sample, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, enc, noise, z, L, latent_dim);
    return launch_status("k_vae_sample");
}

static int seg_args_bad(const char* who, long rows, int C, int cmul, const void* lens, int B, long mul, long div, long s0, long s1) {
    if (rows <= 0 || C <= 0 || C % cmul) return ez_fail(EZDIT_E_INVALID, "%s: rows=%ld must be positive and C=%d a positive multiple of %d", who, rows, C, cmul);
    if (!lens || B <= 0 || mul <= 0 || div <= 0 || s0 <= 0 || s1 <= 0)
        return ez_fail(EZDIT_E_INVALID, "%s: the length table must be given and B=%d, mul=%ld, div=%ld and the sample strides %ld, %ld be positive", who, B, mul, div, s0, s1);
    return EZDIT_OK;
}

int ezvae_snake_bf16_seg(const float* x, int ldx, const float* alpha, const float* inv_beta, void* out, int ldo, long rows, int C,
                         const int32_t* lens, int B, long mul, long div, long stride_in, long stride_out, ezdit_stream stream) {
    if (int rc = seg_args_bad("ezvae_snake_bf16_seg", rows, C, 4, lens, B, mul, div, stride_in, stride_out)) return rc;
    const long total = rows * (C / 4);
    if ((total + 255) / 256 >= (1L << 31)) return ez_fail(EZDIT_E_INVALID, "ezvae_snake_bf16_seg: rows=%ld x C=%d does not fit one launch", rows, C);
    hipLaunchKernelGGL(k_snake_bf16_seg, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, alpha, inv_beta,
                       (bf16_t*)out, ldo, rows, C, lens, B, mul, div, stride_in, stride_out);
    return launch_status("k_snake_bf16_seg");
}

int ezvae_conv_out1_seg(const void* xb, int ldx, const float* w, float* out, long W, int C, const int32_t* lens, int B, long mul, long div,
                        long stride_in, ezdit_stream stream) {
    if (int rc = seg_args_bad("ezvae_conv_out1_seg", W, C, 8, lens, B, mul, div, stride_in, 1)) return rc;
    const long total = W * B;
    if ((total + 255) / 256 >= (1L << 31)) return ez_fail(EZDIT_E_INVALID, "ezvae_conv_out1_seg: B=%d x W=%ld does not fit one launch", B, W);
    hipLaunchKernelGGL(k_conv_out1_seg, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)xb, ldx, w, out, W, C,
                       lens, B, mul, div, stride_in);
    return launch_status("k_conv_out1_seg");
}

int ezvae_conv_in1_seg(const float* wav, const float* w, const float* bias, float* out, long rows, int C, const int32_t* lens, int B, long Tmax,
                       long stride_out, ezdit_stream stream) {
    if (int rc = seg_args_bad("ezvae_conv_in1_seg", rows, C, 4, lens, B, 1, 1, Tmax, stride_out)) return rc;
    const long total = rows * (C / 4);
    if ((total + 255) / 256 >= (1L << 31)) return ez_fail(EZDIT_E_INVALID, "ezvae_conv_in1_seg: rows=%ld x C=%d does not fit one launch", rows, C);
    hipLaunchKernelGGL(k_conv_in1_seg, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, wav, w, bias, out, rows, C, lens, B,
                       Tmax, stride_out);
    return launch_status("k_conv_in1_seg");
}

int ezvae_sample_seg(const float* enc, const float* noise, float* z, int Lmax, int latent_dim, const int32_t* lens, int B, long mul, long div,
                     long stride_enc, ezdit_stream stream) {
    if (int rc = seg_args_bad("ezvae_sample_seg", Lmax, latent_dim, 1, lens, B, mul, div, stride_enc, 1)) return rc;
    if ((long)Lmax * latent_dim >= (1L << 31)) return ez_fail(EZDIT_E_INVALID, "ezvae_sample_seg: Lmax=%d * latent_dim=%d must stay below 2^31", Lmax, latent_dim);
    const long total = (long)Lmax * latent_dim * B;
    if ((total + 255) / 256 >= (1L << 31)) return ez_fail(EZDIT_E_INVALID, "ezvae_sample_seg: B=%d x Lmax=%d x latent_dim=%d does not fit one launch", B, Lmax, latent_dim);
    hipLaunchKernelGGL(k_vae_sample_seg, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, enc, noise, z, Lmax, latent_dim, lens, B,
                       mul, div, stride_enc);
    return launch_status("k_vae_sample_seg");
}

}  // extern "C"
