// Shared prompt passes (ctts_gpt_share_prompts): sequences that name one prompt run it through the prompt pass ONCE, in the KV lane of the first of them (the
// leader); the others (the followers) receive a copy of the leader's prompt span of the cache and of its pending decode-row input.
//
// The cache is [layer][k | v][lane][head][slot][64] of WTraits<WT>::cache_t, so the span [0, span) of one lane is layers x 2 x heads contiguous runs of
// span x 64 elements: span x 256 bytes (fp32 cache) or span x 128 bytes (fp16 cache), whole 16-byte units either way.  The kernel is a byte copy: it moves
// 16-byte units and is the same code for both cache types.
//
// Grid: x = run (layer, k | v, head), y = group, z = a chunk of KS_UNITS units (16 KB) of the run, i.e. sized from the bytes to move -- 20 layers x 8 groups on
// an fp32 cache: a 100-token run is 1600 units = 2 chunks (the second 56 % full), 480 x 8 x 2 = 7680 workgroups; at 400 tokens 6400 units = 7 chunks, 26880
// workgroups.  A workgroup loads its chunk of the leader's run once (KS_UNROLL independent 16-byte loads
// per lane, lane-contiguous: one wave covers 1 KiB per load) and stores it to every follower of the group: (1 + m) chunks of traffic for m followers, not 2 m.
// The group table is read with uniform indices from device memory, so the launch needs no host synchronisation and follows the last prompt pass in stream order.
// Nothing outside [0, span) of the followers' lanes is written; the leader's lane and lanes the table does not name are never written.
#include "kernels.h"

#define KS_THREADS 256
#define KS_UNROLL 4
#define KS_UNITS (KS_THREADS * KS_UNROLL)

__global__ __launch_bounds__(KS_THREADS) void kv_share_kernel(const KvShareArgs a) {
    const int run = blockIdx.x, g = blockIdx.y;
    const int leader = a.groups[3 * g], first = a.groups[3 * g + 1], m = a.groups[3 * g + 2];
    const size_t base = (size_t)(run / a.NH) * a.plane_bytes + (size_t)(run % a.NH) * a.run_bytes;
    const unsigned u0 = blockIdx.z * KS_UNITS + threadIdx.x;
    const uint4* src = (const uint4*)(a.kv + base + (size_t)leader * a.lane_bytes);
    uint4 v[KS_UNROLL];
#pragma unroll
    for (int k = 0; k < KS_UNROLL; ++k) {
        const unsigned u = u0 + k * KS_THREADS;
        if (u < a.units) v[k] = src[u];
    }
    for (int f = 0; f < m; ++f) {
        const int lane = a.followers[first + f];
        uint4* dst = (uint4*)(a.kv + base + (size_t)lane * a.lane_bytes);
#pragma unroll
        for (int k = 0; k < KS_UNROLL; ++k) {
            const unsigned u = u0 + k * KS_THREADS;
            if (u < a.units) dst[u] = v[k];
        }
    }
}
int launch_kv_share(const KvShareArgs& a, int runs, hipStream_t s) {
    if (a.n_groups < 1 || a.units == 0) return 0;
    hipLaunchKernelGGL(kv_share_kernel, dim3(runs, a.n_groups, (a.units + KS_UNITS - 1) / KS_UNITS), dim3(KS_THREADS), 0, s, a);
    CTTS_HIP_CHECK(hipGetLastError());
    return 0;
}

// The pending decode-row input of n sequences: dst[b] <- src[src_idx[b]] (rows of H floats, 16-byte copies).  Default mode: src = dst = the decode rows, src_idx
// = each row's leader (a leader's own row is left alone); batch_invariant: src = the last prompt token's embeddings [prompt][T][H], src_idx = each row's prompt.
__global__ __launch_bounds__(256) void share_rows_kernel(const float* src, size_t src_stride, const int* src_idx, float* dst, int H) {
    const int b = blockIdx.x;
    const float4* sp = (const float4*)(src + (size_t)src_idx[b] * src_stride);
    float4* dp = (float4*)(dst + (size_t)b * H);
    if (sp == dp) return;
    for (int k = threadIdx.x; k < H / 4; k += 256) dp[k] = sp[k];
}
int launch_share_rows(const float* src, size_t src_stride, const int* src_idx, float* dst, int n, int H, hipStream_t s) {
    hipLaunchKernelGGL(share_rows_kernel, dim3(n), dim3(256), 0, s, src, src_stride, src_idx, dst, H);
    CTTS_HIP_CHECK(hipGetLastError());
    return 0;
}
