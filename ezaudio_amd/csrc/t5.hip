// T5 text encoder (flan-t5 family: gated gelu_new feed-forward, head dim 64) behind the ezt5_* section of include/ezdit.h.
// Restates transformers' T5EncoderModel (models/t5/modeling_t5.py: T5LayerNorm, T5Attention with the bidirectional relative-position
// bias of block 0, T5DenseGatedActDense, final_layer_norm) for the text_encoder slot of ezaudio_amd/sampler.py.
//
// One layer is seven launches; the four projections are the bf16 MFMA GEMM of the DiT (csrc/gemm.hip, tile 25, EPI_F32, the
// residual add in its epilogue), exactly as csrc/vae.hip runs its convolutions:
//     u   = bf16(rms(x) w0)                                   k_t5_embed_rms   (layer 0: x = embedding[ids], seeds the stream)
//     qkv = u . [Wq | Wk | Wv]^T                fp32          launch_gemm
//     a   = bf16(softmax(q k^T + bias + mask) v)              k_t5_attn
//     x'  = x + a . Wo^T                        fp32          launch_gemm (resid)
//     u   = bf16(rms(x') w1)                                  k_t5_embed_rms
//     h   = u . [Wi0 | Wi1]^T                   fp32          launch_gemm
//     g   = bf16(gelu_new(h[:, :d_ff]) h[:, d_ff:])           k_t5_gated_gelu
//     x'' = x' + g . Wff^T                      fp32          launch_gemm (resid)
// and the final norm writes fp32.  The residual stream stays fp32 from the embedding to the output (flan-t5 activations reach
// 1e3 - 1e4: a 16-bit stream loses the small updates); bf16 appears only as a GEMM / MFMA operand.
// The tile id does not depend on the row count, and neither kernel below mixes rows of different batch elements, so a row's result
// does not depend on what else is in the batch (tests/test_t5_gpu.py checks it bit for bit).
#include "../../include/ezdit.h"
#include "common.h"
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

struct ezt5_handle {
    ezt5_config cfg;
    int inner;                                // num_heads * d_kv
    std::vector<ezt5_tensor_info_t> tab;
    size_t blob_bytes;
    const char* blob;                         // device, caller-owned (null: not bound)
    char* ws; int B, L;                       // device, caller-owned (null: not bound)
    float *x0, *x1, *qkv, *hff; bf16_t *u, *ao, *g;
};

namespace {

constexpr int T5_GEMM_TILE = 25;   // 128 x 64, 8 waves, ring 4 (csrc/gemm.hip): fp32 output with the residual in the epilogue; the same id for every row count
constexpr int T5_QT = 64;          // queries per workgroup: two waves x 32
constexpr int T5_KT = 64;          // keys per staged tile
constexpr int T5_LDS_LD = 72;      // bf16 elements per LDS row of the K tile ([key][d]) and of the V^T tile ([d][key]): 144 bytes, so the 16 rows a
                                   // ds_read_b128 group touches start 36 banks apart (all distinct mod 64 in steps of 4) instead of on two banks
constexpr int T5_MAX_L = 512;      // the bias row of one head (2 L - 1 floats) lives in LDS

// x fp32 -> bf16(x * rsqrt(mean(x^2) + eps) * w) (T5LayerNorm: no mean, no bias), one wave per row.
//   ids != null: x = emb[ids[row]] and the row is ALSO written to x_out (the fp32 residual stream starts here); else x = x_in[row]
//   out_f32 != null: the result is stored as fp32 there (final_layer_norm) instead of as the bf16 operand u
__global__ __launch_bounds__(256) void k_t5_embed_rms(const int32_t* __restrict__ ids, const float* __restrict__ emb, int vocab,
                                                      const float* x_in, float* x_out /* may be the same buffer: only one of them is touched */, const float* __restrict__ w,
                                                      float eps, bf16_t* __restrict__ u, float* __restrict__ out_f32, int M, int D) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* src;
    if (ids) {
        int id = ids[row];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);   // a token id outside the table must not become an address
        src = emb + (long)id * D;
    } else {
        src = x_in + (long)row * D;
    }
    float ss = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(src + c);
        ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        if (ids) *reinterpret_cast<float4*>(x_out + (long)row * D + c) = v;
    }
    ss = wave_sum(ss);
    const float r = rsqrtf(ss / (float)D + eps);
    for (int c = lane * 4; c < D; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(src + c);
        const float4 g = *reinterpret_cast<const float4*>(w + c);
        const float4 o = make_float4(v.x * r * g.x, v.y * r * g.y, v.z * r * g.z, v.w * r * g.w);
        if (out_f32) {
            *reinterpret_cast<float4*>(out_f32 + (long)row * D + c) = o;
        } else {
            uint2 p;
            p.x = pack_bf2(o.x, o.y);
            p.y = pack_bf2(o.z, o.w);
            *reinterpret_cast<uint2*>(u + (long)row * D + c) = p;
        }
    }
}

__device__ __forceinline__ float gelu_new(float x) {   // transformers NewGELUActivation: the tanh form (EPI_GEGLU's is the erf form)
    return 0.5f * x * (1.f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
}

// h fp32 [M][2 F] (wi_0 columns, then wi_1 columns) -> g bf16 [M][F] = gelu_new(h[:, :F]) * h[:, F:]; one thread per 4 columns
__global__ __launch_bounds__(256) void k_t5_gated_gelu(const float* __restrict__ h, bf16_t* __restrict__ g, long M, int F) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int f4 = F >> 2;
    if (idx >= M * f4) return;
    const long row = idx / f4;
    const int c = (int)(idx % f4) * 4;
    const float4 a = *reinterpret_cast<const float4*>(h + row * 2 * F + c);
    const float4 b = *reinterpret_cast<const float4*>(h + row * 2 * F + F + c);
    uint2 o;
    o.x = pack_bf2(gelu_new(a.x) * b.x, gelu_new(a.y) * b.y);
    o.y = pack_bf2(gelu_new(a.z) * b.z, gelu_new(a.w) * b.w);
    *reinterpret_cast<uint2*>(g + row * F + c) = o;
}

// 8 consecutive operand elements as bf16: from the fp32 projection output (rounded here: the MFMA operand) or from a bf16 buffer (test hook)
template <bool F32IN>
__device__ __forceinline__ uint4 t5_load8(const void* p, long e) {
    if constexpr (F32IN) {
        const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + e);
        const float4 c = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + e + 4);
        return make_uint4(pack_bf2(a.x, a.y), pack_bf2(a.z, a.w), pack_bf2(c.x, c.y), pack_bf2(c.z, c.w));
    } else {
        return *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(p) + e);
    }
}

// T5 self-attention of one (batch element, head, 64-query tile): out = softmax(q k^T + bias[h][key - query] + key mask) v, NO 1 / sqrt(d) scale, head dim 64.
// q / k / v: token-major rows [B L][ld], head h in columns [64 h, 64 h + 64) of each.  Two waves, 32 queries each; keys in tiles of 64 staged through LDS.
// MFMA 32x32x16 bf16 on the TRANSPOSED products, so that in both accumulators a lane owns ONE query (column lane & 31):
//     S^T[key][query] = K[key][:] . Q[query][:]       A operand = K rows (LDS), B operand = Q (registers, loaded once)
//     O^T[d][query]  += V^T[d][keys] . P^T[keys][query]   A operand = V^T rows (LDS, transposed while staging), B operand = P straight from the S registers:
// the contraction runs over the keys in the order the S layout holds them (k-step s2, lane half hi, element e -> key 16 s2 + 8 (e >> 2) + 4 hi + (e & 3)),
// and the V^T fragment is gathered in the same order.  Softmax in fp32 in two passes over the keys (L <= 512: the second Q K^T is cheaper than a
// running rescale and leaves ONE rounding point for P, exp(s - row max), as the emulation in tests/t5_ref.py has it): pass 1 the row maximum over the valid
// keys, pass 2 P, its fp32 row sum and P V.  A key that is masked or >= L is staged as ZEROS in K and V and gets P = 0 by a select, never by arithmetic:
// whatever the buffers hold there (NaN included) cannot reach the output.  A row without any valid key comes out as zeros.  Query rows >= L are not stored.
template <bool F32IN>
__global__ __launch_bounds__(128) void k_t5_attn(const void* __restrict__ q, const void* __restrict__ k, const void* __restrict__ v, int ld,
                                                 const float* __restrict__ bias /* [H][bias_ld], entry (key - query) + bias_half */, int bias_ld, int bias_half,
                                                 const uint8_t* __restrict__ mask /* [B][L], 1 = attend */, bf16_t* __restrict__ out, int ldo, int L) {
    __shared__ __attribute__((aligned(16))) bf16_t sK[T5_KT * T5_LDS_LD];
    __shared__ __attribute__((aligned(16))) bf16_t sV[64 * T5_LDS_LD];
    __shared__ float sBias[2 * T5_MAX_L];
    __shared__ int sValid[T5_KT];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, hi = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    const int qi = blockIdx.x * T5_QT + wave * 32 + r32;
    const int qc = qi < L ? qi : L - 1;   // lanes past the end work on the last row (finite, in bounds) and store nothing
    const long row0 = (long)b * L;

    // bias of this head over the distances -(L - 1) .. L - 1 -> sBias[(key - query) + L - 1]
    for (int i = tid; i < 2 * L - 1; i += 128) sBias[i] = bias[(long)h * bias_ld + bias_half - (L - 1) + i];

    bf16x8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = __builtin_bit_cast(bf16x8, t5_load8<F32IN>(q, (row0 + qc) * ld + h * 64 + ks * 16 + hi * 8));

    const int nkt = (L + T5_KT - 1) / T5_KT;
    auto stage = [&](int kt, bool with_v) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = i * 128 + tid;
            const int r = c >> 3, ch = c & 7;
            const int key = kt * T5_KT + r;
            const bool valid = key < L && mask[row0 + key] != 0;
            const long e = (row0 + (key < L ? key : L - 1)) * ld + h * 64 + ch * 8;
            uint4 kv = make_uint4(0u, 0u, 0u, 0u), vv = kv;
            if (valid) {
                kv = t5_load8<F32IN>(k, e);
                if (with_v) vv = t5_load8<F32IN>(v, e);
            }
            *reinterpret_cast<uint4*>(&sK[r * T5_LDS_LD + ch * 8]) = kv;
            if (with_v) {
                const uint32_t w4[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sV[(ch * 8 + 2 * j) * T5_LDS_LD + r] = (bf16_t)(w4[j] & 0xffffu);
                    sV[(ch * 8 + 2 * j + 1) * T5_LDS_LD + r] = (bf16_t)(w4[j] >> 16);
                }
            }
            if (ch == 0) sValid[r] = valid ? 1 : 0;
        }
    };
    // S^T of the 32-key half `sub` of the staged tile: s[r] belongs to key 32 sub + 8 (r >> 2) + 4 hi + (r & 3)
    auto scores = [&](int kt, int sub, float (&s)[16], bool (&ok)[16]) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&sK[(sub * 32 + r32) * T5_LDS_LD + ks * 16 + hi * 8]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kl = sub * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
            ok[r] = sValid[kl] != 0;
            s[r] = acc[r] + sBias[kt * T5_KT + kl - qc + (L - 1)];   // <= 2 L - 2 for a valid key; an invalid one may read past it (inside the array), unused
        }
    };

    // ---- pass 1: row maximum over the valid keys ----
    float m = -1e30f;
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();
        stage(kt, false);
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            float s[16]; bool ok[16];
            scores(kt, sub, s, ok);
#pragma unroll
            for (int r = 0; r < 16; ++r) m = ok[r] ? fmaxf(m, s[r]) : m;
        }
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));

    // ---- pass 2: P = exp(s - m), row sum, P V ----
    f32x16 o[2];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[f][r] = 0.f;
    float lsum = 0.f;
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();
        stage(kt, true);
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            float s[16]; bool ok[16];
            scores(kt, sub, s, ok);
            float p[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                p[r] = ok[r] ? __expf(s[r] - m) : 0.f;
                lsum += p[r];
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const uint4 pk = make_uint4(pack_bf2(p[8 * s2], p[8 * s2 + 1]), pack_bf2(p[8 * s2 + 2], p[8 * s2 + 3]),
                                            pack_bf2(p[8 * s2 + 4], p[8 * s2 + 5]), pack_bf2(p[8 * s2 + 6], p[8 * s2 + 7]));
                const bf16x8 pf = __builtin_bit_cast(bf16x8, pk);
#pragma unroll
                for (int f = 0; f < 2; ++f) {
                    const bf16_t* vr = &sV[(32 * f + r32) * T5_LDS_LD + sub * 32 + 16 * s2 + 4 * hi];
                    const uint2 lo = *reinterpret_cast<const uint2*>(vr), up = *reinterpret_cast<const uint2*>(vr + 8);
                    const bf16x8 vf = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, up.x, up.y));
                    o[f] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[f], 0, 0, 0);
                }
            }
        }
    }
    lsum += __shfl_xor(lsum, 32, 64);
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
    if (qi < L) {
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint2 w2;
                w2.x = pack_bf2(o[f][4 * g] * inv, o[f][4 * g + 1] * inv);
                w2.y = pack_bf2(o[f][4 * g + 2] * inv, o[f][4 * g + 3] * inv);
                *reinterpret_cast<uint2*>(out + (row0 + qi) * ldo + h * 64 + 32 * f + 8 * g + 4 * hi) = w2;
            }
    }
}

int launch_status(const char* what) {   // a failed launch must surface as an error code, not as stale output
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ez_fail(EZDIT_E_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
    return EZDIT_OK;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The four projections of a layer as (N, K).  What launch_gemm needs of a shape (csrc/gemm.hip: K a positive multiple of BK; common.h stage_offsets: the
// furthest A and W element below 2^31) is decided HERE, by ezt5_bind_workspace, so that ezt5_encode never meets a shape refusal between two launches.
int t5_check_gemm_shape(long M, long N, long K) {
    if (K <= 0 || K % BK || N % 4 || M * K >= (1L << 31) || N * K >= (1L << 31) || M * N >= (1L << 31))
        return ez_fail(EZDIT_E_UNSUPPORTED, "ezt5: the GEMM refuses M=%ld N=%ld K=%ld (K a multiple of %d, every operand below 2^31 elements)", M, N, K, BK);
    return EZDIT_OK;
}

int t5_check_gemm_shapes(const ezt5_handle* h, long M) {
    const long D = h->cfg.d_model, I = h->inner, F = h->cfg.d_ff;
    const long nk[4][2] = {{3 * I, D}, {D, I}, {2 * F, D}, {D, F}};
    for (const auto& s : nk)
        if (int rc = t5_check_gemm_shape(M, s[0], s[1])) return rc;
    return EZDIT_OK;
}

// out fp32 [M][N] = A . W^T (+ resid); nonzero = launch_gemm launched nothing
int t5_gemm(const bf16_t* A, int K, const bf16_t* W, int N, const float* resid, float* out, int M, hipStream_t st) {
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.A = A; g.lda = K; g.W = W; g.ldw = K; g.wrows = N; g.out = out; g.ldo = N; g.M = M; g.N = N; g.K = K;
    g.splitk = 1; g.epi = EPI_F32; g.tile = T5_GEMM_TILE; g.resid = resid; g.ldr = N; g.xcd_map = 1; g.rows_per_b = 1;
    return launch_gemm(g, st);
}

template <bool F32IN>
void launch_t5_attn(const void* q, const void* k, const void* v, int ld, const float* bias, int bias_ld, int bias_half, const uint8_t* mask,
                    bf16_t* out, int ldo, int B, int H, int L, hipStream_t st) {
    hipLaunchKernelGGL(k_t5_attn<F32IN>, dim3((L + T5_QT - 1) / T5_QT, H, B), dim3(128), 0, st, q, k, v, ld, bias, bias_ld, bias_half, mask, out, ldo, L);
}

const ezt5_tensor_info_t* find(const ezt5_handle* h, const char* name) {
    for (const auto& t : h->tab)
        if (!strcmp(t.name, name)) return &t;
    return nullptr;
}

template <class T>
const T* blob_at(const ezt5_handle* h, const char* fmt, int layer) {
    char name[32];
    snprintf(name, sizeof name, fmt, layer);
    const ezt5_tensor_info_t* t = find(h, name);
    return t ? reinterpret_cast<const T*>(h->blob + t->offset) : nullptr;
}

}  // namespace

extern "C" {

int ezt5_create(const ezt5_config* cfg, ezt5_handle** out) {
    if (!cfg || !out) return ez_fail(EZDIT_E_INVALID, "ezt5_create: null argument");
    *out = nullptr;
    const ezt5_config& c = *cfg;
    if (c.vocab <= 0 || c.d_model <= 0 || c.d_kv <= 0 || c.num_heads <= 0 || c.d_ff <= 0 || c.num_layers < 0 || c.num_buckets <= 0 ||
        c.max_distance <= 0 || c.max_len <= 0 || !(c.eps > 0.f))
        return ez_fail(EZDIT_E_INVALID, "ezt5_create: every size must be positive (num_layers may be 0) and eps > 0");
    if (c.d_kv != 64) return ez_fail(EZDIT_E_UNSUPPORTED, "ezt5_create: d_kv=%d, only head dim 64 is built", c.d_kv);
    if (c.ff_act != EZT5_FF_GATED_GELU_NEW)
        return ez_fail(EZDIT_E_UNSUPPORTED, "ezt5_create: feed-forward %d, only the gated gelu_new form (flan-t5 / T5 v1.1) is built", c.ff_act);
    const long inner = (long)c.num_heads * c.d_kv;
    if (c.d_model % 64 || c.d_ff % 64 || inner % 64)
        return ez_fail(EZDIT_E_UNSUPPORTED, "ezt5_create: d_model=%d, d_ff=%d and num_heads * d_kv=%ld must be multiples of 64 (GEMM K tile)", c.d_model, c.d_ff, inner);
    if (c.max_len > T5_MAX_L) return ez_fail(EZDIT_E_UNSUPPORTED, "ezt5_create: max_len=%d, the attention kernel covers up to %d tokens", c.max_len, T5_MAX_L);
    if (c.num_heads > 65535) return ez_fail(EZDIT_E_UNSUPPORTED, "ezt5_create: num_heads=%d exceeds the launch grid", c.num_heads);
    // the staging offsets of the GEMM are 32-bit (csrc/common.h stage_offsets): every weight matrix stays below 2^31 elements
    const long wmax = (long)c.d_model * (3 * inner > 2L * c.d_ff ? 3 * inner : 2L * c.d_ff);
    if (wmax >= (1L << 31) || (long)c.vocab * c.d_model >= (1L << 40))
        return ez_fail(EZDIT_E_UNSUPPORTED, "ezt5_create: a weight matrix of %ld elements does not fit the GEMM's 32-bit staging offset", wmax);
    ezt5_handle* h = new (std::nothrow) ezt5_handle();
    if (!h) return ez_fail(EZDIT_E_INVALID, "ezt5_create: out of host memory");
    h->cfg = c;
    h->inner = (int)inner;
    h->blob = nullptr; h->ws = nullptr; h->B = h->L = 0;
    size_t off = 0;
    auto add = [&](const char* fmt, int layer, int dtype, long rows, long cols) {
        ezt5_tensor_info_t t;
        memset(&t, 0, sizeof t);
        snprintf(t.name, sizeof t.name, fmt, layer);
        t.dtype = dtype; t.rows = rows; t.cols = cols; t.offset = (int64_t)off;
        off = align256(off + (size_t)rows * cols * (dtype == EZDIT_P_BF16 ? 2 : 4));
        h->tab.push_back(t);
    };
    add("embed", 0, EZDIT_P_F32, c.vocab, c.d_model);
    add("bias_table", 0, EZDIT_P_F32, c.num_heads, 2L * c.max_len - 1);
    for (int l = 0; l < c.num_layers; ++l) {
        add("blk%d.ln0", l, EZDIT_P_F32, 1, c.d_model);
        add("blk%d.wqkv", l, EZDIT_P_BF16, 3 * inner, c.d_model);
        add("blk%d.wo", l, EZDIT_P_BF16, c.d_model, inner);
        add("blk%d.ln1", l, EZDIT_P_F32, 1, c.d_model);
        add("blk%d.wi", l, EZDIT_P_BF16, 2L * c.d_ff, c.d_model);
        add("blk%d.wff", l, EZDIT_P_BF16, c.d_model, c.d_ff);
    }
    add("final_ln", 0, EZDIT_P_F32, 1, c.d_model);
    h->blob_bytes = off;
    *out = h;
    return EZDIT_OK;
}

int ezt5_destroy(ezt5_handle* h) {
    delete h;
    return EZDIT_OK;
}

int ezt5_tensor_count(const ezt5_handle* h) { return h ? (int)h->tab.size() : 0; }

size_t ezt5_blob_bytes(const ezt5_handle* h, ezt5_tensor_info_t* table, int capacity) {
    if (!h) { ez_fail(EZDIT_E_INVALID, "ezt5_blob_bytes: null handle"); return 0; }
    if (table)
        for (int i = 0; i < capacity && i < (int)h->tab.size(); ++i) table[i] = h->tab[i];
    return h->blob_bytes;
}

int ezt5_bind_weights(ezt5_handle* h, const void* dev_blob, size_t bytes) {
    if (!h || !dev_blob) return ez_fail(EZDIT_E_INVALID, "ezt5_bind_weights: null argument");
    if (bytes < h->blob_bytes) return ez_fail(EZDIT_E_INVALID, "ezt5_bind_weights: blob of %zu bytes, %zu needed", bytes, h->blob_bytes);
    if ((uintptr_t)dev_blob % 256) return ez_fail(EZDIT_E_INVALID, "ezt5_bind_weights: the blob must be 256-byte aligned");
    h->blob = reinterpret_cast<const char*>(dev_blob);
    return EZDIT_OK;
}

size_t ezt5_workspace_bytes(const ezt5_handle* h, int B, int L) {
    if (!h || B <= 0 || L <= 0) { ez_fail(EZDIT_E_INVALID, "ezt5_workspace_bytes: null handle or B=%d / L=%d not positive", B, L); return 0; }
    if (L > h->cfg.max_len) { ez_fail(EZDIT_E_UNSUPPORTED, "ezt5_workspace_bytes: L=%d exceeds max_len=%d", L, h->cfg.max_len); return 0; }
    const long M = (long)B * L;
    const long wide = 3L * h->inner > 2L * h->cfg.d_ff ? 3L * h->inner : 2L * h->cfg.d_ff;
    if (B > 65535 || M * wide >= (1L << 31)) {   // 32-bit staging offsets of the GEMM operands; attention grid z
        ez_fail(EZDIT_E_UNSUPPORTED, "ezt5_workspace_bytes: B=%d x L=%d rows of %ld columns do not fit the GEMM's 32-bit offsets", B, L, wide);
        return 0;
    }
    const size_t D = h->cfg.d_model, I = h->inner, F = h->cfg.d_ff;
    return 2 * align256(M * D * 4) + align256(M * 3 * I * 4) + align256(M * 2 * F * 4) + align256(M * D * 2) + align256(M * I * 2) + align256(M * F * 2);
}

int ezt5_bind_workspace(ezt5_handle* h, void* dev_ws, size_t bytes, int B, int L) {
    if (!h) return ez_fail(EZDIT_E_INVALID, "ezt5_bind_workspace: null handle");
    const size_t need = ezt5_workspace_bytes(h, B, L);
    if (!need) return B > 0 && L > 0 ? EZDIT_E_UNSUPPORTED : EZDIT_E_INVALID;   // message set above; decided before dev_ws is looked at, so a caller whose size query
    if (!dev_ws) return ez_fail(EZDIT_E_INVALID, "ezt5_bind_workspace: null workspace");   // returned 0 gets the code from here without owning a buffer
    if (bytes < need) return ez_fail(EZDIT_E_INVALID, "ezt5_bind_workspace: %zu bytes, %zu needed for B=%d L=%d", bytes, need, B, L);
    if ((uintptr_t)dev_ws % 256) return ez_fail(EZDIT_E_INVALID, "ezt5_bind_workspace: the workspace must be 256-byte aligned");
    if (int rc = t5_check_gemm_shapes(h, (long)B * L)) return rc;
    const size_t M = (size_t)B * L, D = h->cfg.d_model, I = h->inner, F = h->cfg.d_ff;
    char* p = reinterpret_cast<char*>(dev_ws);
    h->x0 = (float*)p; p += align256(M * D * 4);
    h->x1 = (float*)p; p += align256(M * D * 4);
    h->qkv = (float*)p; p += align256(M * 3 * I * 4);
    h->hff = (float*)p; p += align256(M * 2 * F * 4);
    h->u = (bf16_t*)p; p += align256(M * D * 2);
    h->ao = (bf16_t*)p; p += align256(M * I * 2);
    h->g = (bf16_t*)p;
    h->ws = reinterpret_cast<char*>(dev_ws); h->B = B; h->L = L;
    return EZDIT_OK;
}

int ezt5_encode(ezt5_handle* h, const int32_t* dev_ids, const uint8_t* dev_mask, float* dev_out, int B, int L, ezdit_stream stream) {
    if (!h || !dev_ids || !dev_mask || !dev_out) return ez_fail(EZDIT_E_INVALID, "ezt5_encode: null argument");
    if (B <= 0 || L <= 0) return ez_fail(EZDIT_E_INVALID, "ezt5_encode: B=%d and L=%d must be positive", B, L);
    if (L > h->cfg.max_len) return ez_fail(EZDIT_E_UNSUPPORTED, "ezt5_encode: L=%d exceeds max_len=%d", L, h->cfg.max_len);
    if (!h->blob) return ez_fail(EZDIT_E_STATE, "ezt5_encode: no weights bound (ezt5_bind_weights)");
    if (!h->ws || h->B != B || h->L != L)
        return ez_fail(EZDIT_E_STATE, "ezt5_encode: the workspace is bound for B=%d L=%d, not B=%d L=%d (ezt5_bind_workspace)", h->ws ? h->B : 0, h->ws ? h->L : 0, B, L);
    const ezt5_config& c = h->cfg;
    hipStream_t st = (hipStream_t)stream;
    const int M = B * L, D = c.d_model, I = h->inner, F = c.d_ff;
    const unsigned row_blocks = (unsigned)((M + 3) / 4);
    const float* emb = blob_at<float>(h, "embed", 0);
    const float* bias = blob_at<float>(h, "bias_table", 0);
    const int bias_ld = 2 * c.max_len - 1, bias_half = c.max_len - 1;
    int rc, dev = 0;
    // launch_gemm keeps its per-device kernel attributes in 32 slots and launches nothing on a device beyond them: refuse before the first launch
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) return ez_fail(EZDIT_E_UNSUPPORTED, "ezt5_encode: device index %d, the GEMM covers devices 0 - 31", dev);
    (void)hipGetLastError();
    float *x = h->x0, *xn = h->x1;
    for (int l = 0; l < c.num_layers; ++l) {
        hipLaunchKernelGGL(k_t5_embed_rms, dim3(row_blocks), dim3(256), 0, st, l == 0 ? dev_ids : (const int32_t*)nullptr, emb, c.vocab, (const float*)x, x,
                           blob_at<float>(h, "blk%d.ln0", l), c.eps, h->u, (float*)nullptr, M, D);
        if ((rc = launch_status("k_t5_embed_rms"))) return rc;
        if (t5_gemm(h->u, D, blob_at<bf16_t>(h, "blk%d.wqkv", l), 3 * I, nullptr, h->qkv, M, st))
            return ez_fail(EZDIT_E_HIP, "ezt5_encode: the GEMM M=%d N=%d K=%d was not launched (shape accepted at bind: the runtime refused its LDS attribute)", M, 3 * I, D);
        if ((rc = launch_status("k_gemm (t5 qkv)"))) return rc;
        launch_t5_attn<true>(h->qkv, h->qkv + I, h->qkv + 2 * I, 3 * I, bias, bias_ld, bias_half, dev_mask, h->ao, I, B, c.num_heads, L, st);
        if ((rc = launch_status("k_t5_attn"))) return rc;
        if (t5_gemm(h->ao, I, blob_at<bf16_t>(h, "blk%d.wo", l), D, x, xn, M, st))
            return ez_fail(EZDIT_E_HIP, "ezt5_encode: the GEMM M=%d N=%d K=%d was not launched (shape accepted at bind: the runtime refused its LDS attribute)", M, D, I);
        if ((rc = launch_status("k_gemm (t5 o)"))) return rc;
        hipLaunchKernelGGL(k_t5_embed_rms, dim3(row_blocks), dim3(256), 0, st, (const int32_t*)nullptr, emb, c.vocab, (const float*)xn, xn,
                           blob_at<float>(h, "blk%d.ln1", l), c.eps, h->u, (float*)nullptr, M, D);
        if ((rc = launch_status("k_t5_embed_rms"))) return rc;
        if (t5_gemm(h->u, D, blob_at<bf16_t>(h, "blk%d.wi", l), 2 * F, nullptr, h->hff, M, st))
            return ez_fail(EZDIT_E_HIP, "ezt5_encode: the GEMM M=%d N=%d K=%d was not launched (shape accepted at bind: the runtime refused its LDS attribute)", M, 2 * F, D);
        if ((rc = launch_status("k_gemm (t5 wi)"))) return rc;
        const long total = (long)M * (F / 4);
        hipLaunchKernelGGL(k_t5_gated_gelu, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float*)h->hff, h->g, (long)M, F);
        if ((rc = launch_status("k_t5_gated_gelu"))) return rc;
        if (t5_gemm(h->g, F, blob_at<bf16_t>(h, "blk%d.wff", l), D, xn, x, M, st))
            return ez_fail(EZDIT_E_HIP, "ezt5_encode: the GEMM M=%d N=%d K=%d was not launched (shape accepted at bind: the runtime refused its LDS attribute)", M, D, F);
        if ((rc = launch_status("k_gemm (t5 wff)"))) return rc;
    }
    // final_layer_norm -> fp32 output (a model without layers: straight from the embedding)
    hipLaunchKernelGGL(k_t5_embed_rms, dim3(row_blocks), dim3(256), 0, st, c.num_layers == 0 ? dev_ids : (const int32_t*)nullptr, emb, c.vocab, (const float*)x, x,
                       blob_at<float>(h, "final_ln", 0), c.eps, (bf16_t*)nullptr, dev_out, M, D);
    return launch_status("k_t5_embed_rms (final)");
}

// Everything that bounds an address is refused here, before the first HIP call (as ezdit_test_row and its siblings do): the kernel reads rows of ld elements in
// groups of 8 (16-byte loads of bf16, two of fp32), stores 4 bf16 at a time into rows of ldo, and reads bias[h][bias_half - (L - 1) .. bias_half + L - 1].
int ezt5_test_attention_ex(const void* dev_q, const void* dev_k, const void* dev_v, int f32_in, int ld, const float* dev_bias, int bias_ld, int bias_half,
                           const uint8_t* dev_mask, void* dev_out, int ldo, int B, int H, int L, ezdit_stream stream) {
    if (!dev_q || !dev_k || !dev_v || !dev_bias || !dev_mask || !dev_out) return ez_fail(EZDIT_E_INVALID, "ezt5_test_attention: null argument");
    if (B <= 0 || H <= 0 || L <= 0 || B > 65535 || H > 65535) return ez_fail(EZDIT_E_INVALID, "ezt5_test_attention: B=%d, H=%d, L=%d out of range", B, H, L);
    if (L > T5_MAX_L) return ez_fail(EZDIT_E_UNSUPPORTED, "ezt5_test_attention: L=%d, the kernel covers up to %d tokens", L, T5_MAX_L);
    if (ld < 64 * H || ld % 8) return ez_fail(EZDIT_E_INVALID, "ezt5_test_attention: ld=%d must be a multiple of 8 and at least 64 H = %d", ld, 64 * H);
    if (ldo < 64 * H || ldo % 4) return ez_fail(EZDIT_E_INVALID, "ezt5_test_attention: ldo=%d must be a multiple of 4 and at least 64 H = %d", ldo, 64 * H);
    if (bias_half < L - 1 || bias_ld < bias_half + L)
        return ez_fail(EZDIT_E_INVALID, "ezt5_test_attention: bias_half=%d, bias_ld=%d do not hold the distances -(L - 1) .. L - 1 of L=%d", bias_half, bias_ld, L);
    if ((uintptr_t)dev_q & 15 || (uintptr_t)dev_k & 15 || (uintptr_t)dev_v & 15 || (uintptr_t)dev_out & 7 || (uintptr_t)dev_bias & 3)
        return ez_fail(EZDIT_E_INVALID, "ezt5_test_attention: operands must be 16-byte, the output 8-byte and the bias 4-byte aligned");
    (void)hipGetLastError();
    if (f32_in) launch_t5_attn<true>(dev_q, dev_k, dev_v, ld, dev_bias, bias_ld, bias_half, dev_mask, (bf16_t*)dev_out, ldo, B, H, L, (hipStream_t)stream);
    else launch_t5_attn<false>(dev_q, dev_k, dev_v, ld, dev_bias, bias_ld, bias_half, dev_mask, (bf16_t*)dev_out, ldo, B, H, L, (hipStream_t)stream);
    return launch_status("k_t5_attn");
}

int ezt5_test_attention(const void* dev_q, const void* dev_k, const void* dev_v, const float* dev_bias, const uint8_t* dev_mask, void* dev_out,
                        int B, int H, int L, ezdit_stream stream) {
    if (H <= 0 || H > 65535 || L <= 0) return ez_fail(EZDIT_E_INVALID, "ezt5_test_attention: B=%d, H=%d, L=%d out of range", B, H, L);
    return ezt5_test_attention_ex(dev_q, dev_k, dev_v, 0, H * 64, dev_bias, 2 * L - 1, L - 1, dev_mask, dev_out, H * 64, B, H, L, stream);
}

int ezt5_test_embed_rms(const int32_t* dev_ids, const float* dev_emb, int vocab, const float* dev_x_in, float* dev_x_out, const float* dev_w, float eps,
                        void* dev_u_bf16, float* dev_out_f32, int M, int D, ezdit_stream stream) {
    if (!dev_w) return ez_fail(EZDIT_E_INVALID, "ezt5_test_embed_rms: null weight");
    if ((dev_ids != nullptr) == (dev_x_in != nullptr)) return ez_fail(EZDIT_E_INVALID, "ezt5_test_embed_rms: exactly one of ids / x_in");
    if ((dev_u_bf16 != nullptr) == (dev_out_f32 != nullptr)) return ez_fail(EZDIT_E_INVALID, "ezt5_test_embed_rms: exactly one of u_bf16 / out_f32");
    if (dev_ids && (!dev_emb || !dev_x_out || vocab <= 0)) return ez_fail(EZDIT_E_INVALID, "ezt5_test_embed_rms: ids need emb, x_out and vocab=%d > 0", vocab);
    if (M <= 0 || D <= 0 || D % 4) return ez_fail(EZDIT_E_INVALID, "ezt5_test_embed_rms: M=%d must be positive and D=%d a positive multiple of 4", M, D);
    if ((uintptr_t)dev_emb & 15 || (uintptr_t)dev_x_in & 15 || (uintptr_t)dev_x_out & 15 || (uintptr_t)dev_w & 15 || (uintptr_t)dev_u_bf16 & 7 || (uintptr_t)dev_out_f32 & 15)
        return ez_fail(EZDIT_E_INVALID, "ezt5_test_embed_rms: fp32 buffers must be 16-byte, the bf16 output 8-byte aligned");
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_t5_embed_rms, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dev_ids, dev_emb, vocab, dev_x_in, dev_x_out, dev_w, eps,
                       (bf16_t*)dev_u_bf16, dev_out_f32, M, D);
    return launch_status("k_t5_embed_rms");
}

int ezt5_test_gated_gelu(const float* dev_h, void* dev_g, int M, int F, ezdit_stream stream) {
    if (!dev_h || !dev_g) return ez_fail(EZDIT_E_INVALID, "ezt5_test_gated_gelu: null argument");
    if (M <= 0 || F <= 0 || F % 4) return ez_fail(EZDIT_E_INVALID, "ezt5_test_gated_gelu: M=%d must be positive and F=%d a positive multiple of 4", M, F);
    if ((uintptr_t)dev_h & 15 || (uintptr_t)dev_g & 7) return ez_fail(EZDIT_E_INVALID, "ezt5_test_gated_gelu: h must be 16-byte, g 8-byte aligned");
    (void)hipGetLastError();
    const long total = (long)M * (F / 4);
    hipLaunchKernelGGL(k_t5_gated_gelu, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dev_h, (bf16_t*)dev_g, (long)M, F);
    return launch_status("k_t5_gated_gelu");
}

int ezt5_test_gemm(const void* dev_A, int K, const void* dev_W, int N, const float* dev_resid, float* dev_out, int M, ezdit_stream stream) {
    if (!dev_A || !dev_W || !dev_out) return ez_fail(EZDIT_E_INVALID, "ezt5_test_gemm: null argument");
    if (M <= 0 || N <= 0) return ez_fail(EZDIT_E_INVALID, "ezt5_test_gemm: M=%d and N=%d must be positive", M, N);
    if (int rc = t5_check_gemm_shape(M, N, K)) return rc;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) return ez_fail(EZDIT_E_UNSUPPORTED, "ezt5_test_gemm: device index %d, the GEMM covers devices 0 - 31", dev);
    (void)hipGetLastError();
    if (t5_gemm((const bf16_t*)dev_A, K, (const bf16_t*)dev_W, N, dev_resid, dev_out, M, (hipStream_t)stream))
        return ez_fail(EZDIT_E_HIP, "ezt5_test_gemm: the GEMM M=%d N=%d K=%d was not launched", M, N, K);
    return launch_status("k_gemm (t5 hook)");
}

int ezt5_test_rms(const float* dev_x, const float* dev_w, float eps, void* dev_out, int M, int D, ezdit_stream stream) {
    if (!dev_x || !dev_w || !dev_out) return ez_fail(EZDIT_E_INVALID, "ezt5_test_rms: null argument");
    if (M <= 0 || D <= 0 || D % 4) return ez_fail(EZDIT_E_INVALID, "ezt5_test_rms: M=%d must be positive and D=%d a positive multiple of 4", M, D);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_t5_embed_rms, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const int32_t*)nullptr, (const float*)nullptr, 0,
                       dev_x, (float*)nullptr, dev_w, eps, (bf16_t*)dev_out, (float*)nullptr, M, D);
    return launch_status("k_t5_embed_rms");
}

}  // extern "C"
