// Teacher-forced scoring of audio codes (ctts_gpt_score, gpt_engine.hip): after each prompt pass the rows that predict a target are gathered into a
// contiguous block, the final RMSNorm + 4 folded code heads run on it (skinny_gemm.hip PRO_NORM / EPI_LOGITS), and one wave per (row, codebook)
// reduces the row's 626 raw logits to log_softmax at the target and the first argmax (train_lora.py:443-469 restated per entry).
#include "kernels.h"

// gathered row g of a pass -> its sequence: the largest b with cum[b] <= g (sequences without rows in this pass have cum[b] == cum[b + 1])
__device__ inline int score_seq_of(const ScoreRows& sr, int g) {
    int lo = 0, hi = sr.B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sr.cum[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// rows g0 .. g0 + m - 1 of the pass's scored block: x_pre row -> dst[g - g0]; oidx[g - g0] = b * max_targets + j (the output entry it predicts)
__global__ __launch_bounds__(192) void score_gather_kernel(const float* src, float* dst, int* oidx, int g0, const ScoreRows sr) {
    const int i = blockIdx.x, g = g0 + i;
    const int b = score_seq_of(sr, g);
    const int k = g - sr.cum[b];
    const int src_row = sr.first[b] + k;                  // row in the pass (first[b] >= 0: the host clipped it to the pass)
    const f32x4* s = (const f32x4*)(src + (size_t)src_row * 768);
    ((f32x4*)(dst + (size_t)i * 768))[threadIdx.x] = s[threadIdx.x];
    if (threadIdx.x == 0) oidx[i] = b * sr.max_targets + sr.j0[b] + k;
}

// one wave per (row, codebook): max, sum of exp in fp32 (precise expf / logf), the target's log-probability, the first argmax.
// A target outside [0, V) gives NaN and -1 and reads no logit.
__global__ __launch_bounds__(256) void score_reduce_kernel(const float* logits, const int* oidx, const int* targets, float* logprob, int* argmax,
                                                           int m, int V, int n_valid) {
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int i = w >> 2, c = w & 3;
    if (i >= m) return;
    const float* lg = logits + (size_t)i * n_valid + (size_t)c * V;
    const int o = oidx[i] * CTTS_NUM_VQ + c;
    const int t = targets[o];
    // first index of the largest logit: key = order-preserving float bits | ~index (ties -> the smaller index; NaN ranks above +inf, as in torch.argmax)
    unsigned long long best = 0ull;
    for (int k = lane; k < V; k += 64) {
        const unsigned long long key = ((unsigned long long)f32_key(lg[k]) << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)k);
        best = umax64(best, key);
    }
    best = wave_max_u64(best);
    const float mx = key_f32((unsigned)(best >> 32));
    const int am = (int)(0xFFFFFFFFu - (unsigned)best);
    float s = 0.f;
    for (int k = lane; k < V; k += 64) s += expf(lg[k] - mx);
    s = wave_sum(s);
    if (lane == 0) {
        const bool ok = (t >= 0 && t < V);
        logprob[o] = ok ? (lg[ok ? t : 0] - mx) - logf(s) : __builtin_nanf("");
        argmax[o] = ok ? am : -1;
    }
}

// ctts_gpt_score_text: one row of V (21178) raw text-head logits per workgroup of 4 waves.  The same reduction as above a level higher: per thread a strided
// pass for the key of the first largest logit (f32_key | ~index), the wave reduction, the 4 wave results through LDS in wave order; then sum expf(lg - mx) in fp32
// the same way (thread: ascending k; wave_sum; waves 0..3 in order -- a fixed order, so a row's value does not depend on the rows beside it).
// A target outside [0, V) gives NaN and -1 and reads no logit.
__global__ __launch_bounds__(256) void score_text_reduce_kernel(const float* logits, const int* oidx, const int* targets, float* logprob, int* argmax, int V) {
    __shared__ unsigned long long key_s[4];
    __shared__ float sum_s[4];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* lg = logits + (size_t)i * V;
    unsigned long long best = 0ull;
    for (int k = tid; k < V; k += 256) {
        const unsigned long long key = ((unsigned long long)f32_key(lg[k]) << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)k);
        best = umax64(best, key);
    }
    best = wave_max_u64(best);
    if (lane == 0) key_s[wave] = best;
    __syncthreads();
    best = umax64(umax64(key_s[0], key_s[1]), umax64(key_s[2], key_s[3]));
    const float mx = key_f32((unsigned)(best >> 32));
    const int am = (int)(0xFFFFFFFFu - (unsigned)best);
    float s = 0.f;
    for (int k = tid; k < V; k += 256) s += expf(lg[k] - mx);
    s = wave_sum(s);
    if (lane == 0) sum_s[wave] = s;
    __syncthreads();
    if (tid == 0) {
        s = ((sum_s[0] + sum_s[1]) + sum_s[2]) + sum_s[3];
        const int o = oidx[i];
        const int t = targets[o];
        const bool ok = (t >= 0 && t < V);
        logprob[o] = ok ? (lg[ok ? t : 0] - mx) - logf(s) : __builtin_nanf("");
        argmax[o] = ok ? am : -1;
    }
}

int launch_score_text_reduce(const float* logits, const int* oidx, const int* targets, float* logprob, int* argmax, int m, int V, hipStream_t s) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(score_text_reduce_kernel, dim3(m), dim3(256), 0, s, logits, oidx, targets, logprob, argmax, V);
    CTTS_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_score_gather(const float* x_pre, float* dst, int* oidx, int g0, int m, const ScoreRows& sr, hipStream_t s) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(score_gather_kernel, dim3(m), dim3(192), 0, s, x_pre, dst, oidx, g0, sr);
    CTTS_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_score_reduce(const float* logits, const int* oidx, const int* targets, float* logprob, int* argmax, int m, int V, int n_valid, hipStream_t s) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(score_reduce_kernel, dim3(m), dim3(256), 0, s, logits, oidx, targets, logprob, argmax, m, V, n_valid);
    CTTS_HIP_CHECK(hipGetLastError());
    return 0;
}
