// Per-utterance LoRA: adapters that stay SEPARATE from the packed weights, one (or none) per sequence of a batch.
//
// The reference serves an adapter by merging it into a deep copy of the whole Llama for the call (peft merge_and_unload,
// pipelines/chattts_plus_pipeline.py:420-432: W' = W + (alpha / r) B A on every nn.Linear the adapter names) -- one adapter per batch.
// Here  y = W x + scale * B (A x)  is evaluated per row: a small kernel per projection group computes the low-rank term of every
// row with the row's own adapter (rows of sequences without one get zeros) and the projection kernels add it in their epilogues
// (before RoPE / the cache append for q/k/v, with the residual for o_proj).  Two extra launches per layer, paid only by batches
// that carry adapters; the algebra equals the merged weights up to fp32 rounding.
// The MLP projections (gate_proj / up_proj / down_proj) work the same way from tables of their own (second half of this file): two more launches per layer while a
// live row's adapter names one of them.
#include "kernels.h"

#define LORA_RMAX 16

__device__ inline float block_sum_256(float v, float* red, int tid) {
    v = wave_sum(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    const float s = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return s;
}

// One block = one (row, target): 4 waves x 4 rank components, every lane owns 12 of the 768 input columns.  All loads of a phase are
// issued together (a first version walked the 16 dot products one after the other, each waiting for its own loads: 20-40 us per
// launch, 3.7x the step time at batch 32).
// ldb = floats between two rank rows of B_t (the target's output width); the block writes 768 outputs.
__device__ inline void lora_low_rank(const float* hw, const float* A_t, const float* B_t, float scale, float* drow, int H, float* u, int tid, int ldb) {
    const int lane = tid & 63, wave = tid >> 6;
    float hv[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) hv[i] = hw[lane + 64 * i];
    float acc[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {                      // rank components 4 * wave + kk
        const float* ar = A_t + (size_t)(4 * wave + kk) * H + lane;
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < 12; ++i) a += ar[64 * i] * hv[i];
        acc[kk] = a;
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) { const float v = wave_sum(acc[kk]); if (lane == 0) u[4 * wave + kk] = v; }
    __syncthreads();
    float uu[LORA_RMAX];
#pragma unroll
    for (int k = 0; k < LORA_RMAX; ++k) uu[k] = u[k];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int n = tid + 256 * i;
        float b[LORA_RMAX];                                   // B is stored rank-major [16][768]
#pragma unroll
        for (int k = 0; k < LORA_RMAX; ++k) b[k] = B_t[(size_t)k * ldb + n];
        float a = 0.f;
        a += b[0] * uu[0] + b[1] * uu[1] + b[2] * uu[2] + b[3] * uu[3];
        a += b[4] * uu[4] + b[5] * uu[5] + b[6] * uu[6] + b[7] * uu[7];
        a += b[8] * uu[8] + b[9] * uu[9] + b[10] * uu[10] + b[11] * uu[11];
        a += b[12] * uu[12] + b[13] * uu[13] + b[14] * uu[14] + b[15] * uu[15];
        drow[n] = scale * a;
    }
}

// q/k/v targets: input = input_layernorm(x) (llama.py:726-731: the projections see the normalised hidden states)
//   x [rows][768] fp32 residual stream, lnw [768], meta row -> sequence, slot_of_seq [max_batch] (-1 = no adapter),
//   A_l / B_l: this layer's adapters, [slot][target 0..3][16][768], both rank-major (B transposed; zero padded to r = 16), scale_l [slot][4]
//   delta [rows][3][768];  grid = (rows, 3 targets)
__global__ __launch_bounds__(256) void lora_delta_qkv_kernel(const float* x, const float* lnw, float eps, const RowMeta* meta, const int* slot_of_seq,
                                                           const float* A_l, const float* B_l, const float* scale_l, float* delta, int H) {
    __shared__ float hw[768];
    __shared__ float u[LORA_RMAX];
    __shared__ float red[4];
    const int r = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int slot = slot_of_seq[meta[r].seq];
    float* drow = delta + ((size_t)r * 3 + t) * H;
    if (slot < 0) {
        for (int i = tid; i < H; i += 256) drow[i] = 0.f;
        return;
    }
    float xv[3], ss = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) { xv[i] = x[(size_t)r * H + tid + 256 * i]; ss += xv[i] * xv[i]; }
    ss = block_sum_256(ss, red, tid);
    const float rs = 1.0f / sqrtf(ss / (float)H + eps);                  // LlamaRMSNorm (llama.py:82-87)
#pragma unroll
    for (int i = 0; i < 3; ++i) hw[tid + 256 * i] = lnw[tid + 256 * i] * (xv[i] * rs);
    __syncthreads();
    const size_t off = ((size_t)slot * 4 + t) * LORA_RMAX * H;
    lora_low_rank(hw, A_l + off, B_l + off, scale_l[slot * 4 + t], drow, H, u, tid, H);
}

// o_proj target: input = the attention output rows, read back from the o_proj kernel's fragment-major B operand (S = 1 path)
template <typename WT>
__global__ __launch_bounds__(256) void lora_delta_o_kernel(const void* attn_packed, int nbg, const RowMeta* meta, const int* slot_of_seq, const float* A_l,
                                                         const float* B_l, const float* scale_l, float* delta, int H) {
    __shared__ float o[768];
    __shared__ float u[LORA_RMAX];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int slot = slot_of_seq[meta[r].seq];
    float* drow = delta + (size_t)r * H;
    if (slot < 0) {
        for (int i = tid; i < H; i += 256) drow[i] = 0.f;
        return;
    }
    constexpr int KT = WTraits<WT>::KT, EPL = WTraits<WT>::EPL;
    const int NB = 16 * nbg, kt = H / KT;
    const WT* base = (const WT*)attn_packed + (size_t)(r / NB) * nbg * kt * 64 * EPL;
#pragma unroll
    for (int i = 0; i < 3; ++i) { const int c = tid + 256 * i; o[c] = (float)base[xfrag_index<WT>(r % NB, c, kt)]; }
    __syncthreads();
    const size_t off = ((size_t)slot * 4 + 3) * LORA_RMAX * H;
    lora_low_rank(o, A_l + off, B_l + off, scale_l[slot * 4 + 3], drow, H, u, tid, H);
}

// the same for the parity engine's split prompt pass (prefill_split.hip): the attention output rows exist as head / tail fp16 images [16-row group][24 k-tiles][lane][16 B]
__global__ __launch_bounds__(256) void lora_delta_o_split_kernel(const half_t* hi, const half_t* lo, const RowMeta* meta, const int* slot_of_seq, const float* A_l,
                                                               const float* B_l, const float* scale_l, float* delta, int H) {
    __shared__ float o[768];
    __shared__ float u[LORA_RMAX];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int slot = slot_of_seq[meta[r].seq];
    float* drow = delta + (size_t)r * H;
    if (slot < 0) {
        for (int i = tid; i < H; i += 256) drow[i] = 0.f;
        return;
    }
    const size_t base = (size_t)(r >> 4) * 24 * 64 * 8;
#pragma unroll
    for (int i = 0; i < 3; ++i) { const int c = tid + 256 * i; const size_t q = base + xfrag_index<half_t>(r & 15, c, 24); o[c] = (float)hi[q] + (float)lo[q]; }
    __syncthreads();
    const size_t off = ((size_t)slot * 4 + 3) * LORA_RMAX * H;
    lora_low_rank(o, A_l + off, B_l + off, scale_l[slot * 4 + 3], drow, H, u, tid, H);
}
int launch_lora_delta_o_split(const void* hi, const void* lo, const RowMeta* meta, const int* slot_of_seq, const float* A_l, const float* B_l,
                              const float* scale_l, float* delta, int rows, int H, hipStream_t s) {
    if (H != 768) { ctts_set_error("lora: hidden %d != 768", H); return 1; }
    hipLaunchKernelGGL(lora_delta_o_split_kernel, dim3(rows), dim3(256), 0, s, (const half_t*)hi, (const half_t*)lo, meta, slot_of_seq, A_l, B_l, scale_l, delta, H);
    CTTS_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_lora_delta_qkv(const float* x, const float* lnw, float eps, const RowMeta* meta, const int* slot_of_seq, const float* A_l, const float* B_l,
                          const float* scale_l, float* delta, int rows, int H, hipStream_t s) {
    if (H != 768) { ctts_set_error("lora: hidden %d != 768", H); return 1; }
    hipLaunchKernelGGL(lora_delta_qkv_kernel, dim3(rows, 3), dim3(256), 0, s, x, lnw, eps, meta, slot_of_seq, A_l, B_l, scale_l, delta, H);
    CTTS_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_lora_delta_o(int dtype, const void* attn_packed, int nbg, const RowMeta* meta, const int* slot_of_seq, const float* A_l, const float* B_l,
                        const float* scale_l, float* delta, int rows, int H, hipStream_t s) {
    if (dtype == 1) hipLaunchKernelGGL(lora_delta_o_kernel<half_t>, dim3(rows), dim3(256), 0, s, attn_packed, nbg, meta, slot_of_seq, A_l, B_l, scale_l, delta, H);
    else hipLaunchKernelGGL(lora_delta_o_kernel<float>, dim3(rows), dim3(256), 0, s, attn_packed, nbg, meta, slot_of_seq, A_l, B_l, scale_l, delta, H);
    CTTS_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- MLP targets (gate_proj / up_proj / down_proj, llama.py:214,737-739) ------------------------------------------------------------
// Their tables are separate from the q/k/v/o ones (allocated when the first MLP target is loaded, gpt_engine.hip lora_ensure_mlp_storage):
//   A_gu [slot][gate | up][16][768], B_gu [slot][gate | up][16][3072], A_d [slot][16][3072], B_d [slot][16][768], scale_l [slot][4] = gate, up, down, -
#define LORA_I 3072

// gate / up targets: input = post_attention_layernorm(x) (llama.py:737-738).  delta [rows][gate | up][3072]: the SwiGLU epilogues add it BEFORE the
// activation, act = silu(g + dg) * (u + du).  grid = (rows, 2 targets x 4 quarters of the 3072 outputs): every block normalises the row and forms u = A h itself
// (48 KB of A from L2) and writes 768 outputs -- lora_delta_qkv_kernel's shape, four times, instead of one block walking 12 output batches in a row.
__global__ __launch_bounds__(256) void lora_delta_gu_kernel(const float* x, const float* lnw, float eps, const RowMeta* meta, const int* slot_of_seq,
                                                          const float* A_l, const float* B_l, const float* scale_l, float* delta, int H) {
    __shared__ float hw[768];
    __shared__ float u[LORA_RMAX];
    __shared__ float red[4];
    const int r = blockIdx.x, t = blockIdx.y >> 2, q = blockIdx.y & 3, tid = threadIdx.x;
    const int slot = slot_of_seq[meta[r].seq];
    float* drow = delta + ((size_t)r * 2 + t) * LORA_I + q * 768;
    if (slot < 0) {
        for (int i = tid; i < 768; i += 256) drow[i] = 0.f;
        return;
    }
    float xv[3], ss = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) { xv[i] = x[(size_t)r * H + tid + 256 * i]; ss += xv[i] * xv[i]; }
    ss = block_sum_256(ss, red, tid);
    const float rs = 1.0f / sqrtf(ss / (float)H + eps);                  // LlamaRMSNorm (llama.py:82-87)
#pragma unroll
    for (int i = 0; i < 3; ++i) hw[tid + 256 * i] = lnw[tid + 256 * i] * (xv[i] * rs);
    __syncthreads();
    const size_t st = (size_t)slot * 2 + t;
    lora_low_rank(hw, A_l + st * LORA_RMAX * H, B_l + st * LORA_RMAX * LORA_I + q * 768, scale_l[slot * 4 + t], drow, H, u, tid, LORA_I);
}

// down target: 16 waves = 4 quarters of the 3072 inputs x 4 groups of 4 rank components, lora_low_rank's register shape per wave (12 inputs per lane, 48 loads of A in
// flight); the quarters' partial dot products are added in quarter order (deterministic), then 768 threads finish one output each.
// av = this lane's inputs kq * 768 + lane + 64 i, i < 12
__device__ inline void lora_low_rank_down(const float (&av)[12], const float* A_t, const float* B_t, float scale, float* drow, float (*up)[LORA_RMAX], int tid) {
    const int lane = tid & 63, wave = tid >> 6, kq = wave & 3, rg = wave >> 2;
    float acc[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const float* ar = A_t + (size_t)(4 * rg + kk) * LORA_I + kq * 768 + lane;
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < 12; ++i) a += ar[64 * i] * av[i];
        acc[kk] = a;
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) { const float v = wave_sum(acc[kk]); if (lane == 0) up[kq][4 * rg + kk] = v; }
    __syncthreads();
    if (tid >= 768) return;
    float b[LORA_RMAX];                                       // B is stored rank-major [16][768]
#pragma unroll
    for (int k = 0; k < LORA_RMAX; ++k) b[k] = B_t[(size_t)k * 768 + tid];
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < LORA_RMAX; ++k) a += b[k] * (((up[0][k] + up[1][k]) + up[2][k]) + up[3][k]);
    drow[tid] = scale * a;
}

// input = silu(gate) * up as the down projection itself reads it: the SwiGLU epilogue's fragment-major packed copy in the engine dtype (fp16 engines: the saturated fp16
// values -- recomputing them in fp32 would leave "fused == merged" at the mercy of that rounding)
template <typename WT>
__global__ __launch_bounds__(1024) void lora_delta_down_kernel(const void* act_packed, int nbg, const RowMeta* meta, const int* slot_of_seq, const float* A_l,
                                                             const float* B_l, const float* scale_l, float* delta) {
    __shared__ float up[4][LORA_RMAX];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int slot = slot_of_seq[meta[r].seq];
    float* drow = delta + (size_t)r * 768;
    if (slot < 0) {
        if (tid < 768) drow[tid] = 0.f;
        return;
    }
    constexpr int KT = WTraits<WT>::KT, EPL = WTraits<WT>::EPL;
    const int NB = 16 * nbg, kt = LORA_I / KT;
    const WT* base = (const WT*)act_packed + (size_t)(r / NB) * nbg * kt * 64 * EPL;
    const int c0 = ((tid >> 6) & 3) * 768 + (tid & 63);
    float av[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) av[i] = (float)base[xfrag_index<WT>(r % NB, c0 + 64 * i, kt)];
    lora_low_rank_down(av, A_l + (size_t)slot * LORA_RMAX * LORA_I, B_l + (size_t)slot * LORA_RMAX * 768, scale_l[slot * 4 + 2], drow, up, tid);
}

// the same for the parity engine's split prompt pass: the SwiGLU epilogue of prefill_split.hip left head / tail fp16 images [16-row group][96 k-tiles][lane][16 B] of
// silu(g) * u / CTTS_SPLIT_ACT_SCALE
__global__ __launch_bounds__(1024) void lora_delta_down_split_kernel(const half_t* hi, const half_t* lo, const RowMeta* meta, const int* slot_of_seq, const float* A_l,
                                                                   const float* B_l, const float* scale_l, float* delta) {
    __shared__ float up[4][LORA_RMAX];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int slot = slot_of_seq[meta[r].seq];
    float* drow = delta + (size_t)r * 768;
    if (slot < 0) {
        if (tid < 768) drow[tid] = 0.f;
        return;
    }
    const size_t base = (size_t)(r >> 4) * (LORA_I / 32) * 64 * 8;
    const int c0 = ((tid >> 6) & 3) * 768 + (tid & 63);
    float av[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) { const size_t q = base + xfrag_index<half_t>(r & 15, c0 + 64 * i, LORA_I / 32); av[i] = ((float)hi[q] + (float)lo[q]) * CTTS_SPLIT_ACT_SCALE; }
    lora_low_rank_down(av, A_l + (size_t)slot * LORA_RMAX * LORA_I, B_l + (size_t)slot * LORA_RMAX * 768, scale_l[slot * 4 + 2], drow, up, tid);
}

int launch_lora_delta_gu(const float* x, const float* lnw, float eps, const RowMeta* meta, const int* slot_of_seq, const float* A_l, const float* B_l,
                         const float* scale_l, float* delta, int rows, int H, int I, hipStream_t s) {
    if (H != 768 || I != LORA_I) { ctts_set_error("lora: hidden %d / intermediate %d != 768 / %d", H, I, LORA_I); return 1; }
    hipLaunchKernelGGL(lora_delta_gu_kernel, dim3(rows, 8), dim3(256), 0, s, x, lnw, eps, meta, slot_of_seq, A_l, B_l, scale_l, delta, H);
    CTTS_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_lora_delta_down(int dtype, const void* act_packed, int nbg, const RowMeta* meta, const int* slot_of_seq, const float* A_l, const float* B_l,
                           const float* scale_l, float* delta, int rows, int H, int I, hipStream_t s) {
    if (H != 768 || I != LORA_I) { ctts_set_error("lora: hidden %d / intermediate %d != 768 / %d", H, I, LORA_I); return 1; }
    if (dtype == 1) hipLaunchKernelGGL(lora_delta_down_kernel<half_t>, dim3(rows), dim3(1024), 0, s, act_packed, nbg, meta, slot_of_seq, A_l, B_l, scale_l, delta);
    else hipLaunchKernelGGL(lora_delta_down_kernel<float>, dim3(rows), dim3(1024), 0, s, act_packed, nbg, meta, slot_of_seq, A_l, B_l, scale_l, delta);
    CTTS_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_lora_delta_down_split(const void* hi, const void* lo, const RowMeta* meta, const int* slot_of_seq, const float* A_l, const float* B_l,
                                 const float* scale_l, float* delta, int rows, int H, int I, hipStream_t s) {
    if (H != 768 || I != LORA_I) { ctts_set_error("lora: hidden %d / intermediate %d != 768 / %d", H, I, LORA_I); return 1; }
    hipLaunchKernelGGL(lora_delta_down_split_kernel, dim3(rows), dim3(1024), 0, s, (const half_t*)hi, (const half_t*)lo, meta, slot_of_seq, A_l, B_l, scale_l, delta);
    CTTS_HIP_CHECK(hipGetLastError());
    return 0;
}
