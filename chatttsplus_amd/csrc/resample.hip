// Output sample rate on gfx950: torchaudio.functional.resample (sinc_interp_hann, the algorithm chatttsplus_amd/audio.py restates; the reference
// uses it on the input side, pipelines/chattts_plus_pipeline.py:495) for the waveforms and streaming windows that leave the engine.
//
// Arithmetic: a rate pair reduced by its gcd is orig : new.  Output frame i holds the `new` samples j = i new + p, p = 0 .. new-1,
//   y[j] = sum_{k < K} kernels[p][k] x[i orig - width + k],     K = 2 width + orig,  x = 0 outside [0, n)
// (audio.resample's strided conv1d over the zero-padded waveform).  The table comes from Python (audio.resample_kernels) and is kept transposed,
// tab[k][p], so that lanes on consecutive phases read consecutive words.
//
// One launch serves every window of a call: blockIdx.y = window, blockIdx.x = tile of F = RS_R G output frames counted from frame 0 of the
// WAVEFORM (not of the window), so a window is cut at the same frames whatever its j0.  A workgroup stages the tile's input span
// F orig + 2 width in LDS (dynamic: 4 - 12 KB at the rates in use, so 8 workgroups share a CU) (zeros outside [0, total) and outside the caller's buffer) and, for a table of at most RS_TS words, the table; larger
// tables (the 147-phase rates: 54 - 100 KB) are read through L1 / L2.  A thread owns phases ph, ph + ceil(new / 2) of frames g + r G, r < RS_R: per tap two
// table words and RS_R input words feed 2 RS_R accumulators (the kernel is bound by those reads, not by its bytes); the input words are LDS reads at
// lane stride 0 (lanes on one frame: broadcast) or `orig` words only when new < 64 -- 3 : 1,
// 3 : 2, 1 : 2 are odd or unit strides, free of bank conflicts; the strides 160 and 80 of the 147-phase rates never occur between lanes.
//
// Every output is ONE chain acc = fmaf(tab[k][p], x_k, acc), k ascending over all K taps, from acc = 0: no split sums, no tap skipped (a tap outside
// the waveform enters as 0.0f).  Nothing in the chain depends on j0, src0, the tile or B, so a sample has the same bits in every window and batch.
#include <vector>

#include "common.h"
#include "roctx_range.h"
#include "../../include/ctts_hip.h"

#define RS_THREADS 256
#define RS_R 4               // output frames per thread (register blocking: one table word, RS_R fmaf)
#define RS_XS 8192           // words of input span a tile may stage
#define RS_TS 4096           // a table of at most this many words is staged in LDS
#define RS_ITEMS 256         // (phase pair, frame group) items a tile aims at: one per thread (small tiles: a streaming call is a few workgroups deep)

struct RsWin { const float* src; long long src0, total, j0, out_off; int src_n, count; };
#define RS_TAB_BYTES ((size_t)CTTS_RESAMPLE_MAX_WINDOWS * sizeof(RsWin))

struct ctts_resampler {
    int orig = 0, new_ = 0, width = 0, K = 0, G = 1;
    float* d_tab = nullptr;          // [K][new]
    RsWin* d_win = nullptr;
    char* pin = nullptr;
    hipEvent_t pin_ev[4] = {};
    bool pin_used[4] = {};
    int pin_next = 0;
};

template <bool TAB_LDS, int RP>
__global__ __launch_bounds__(RS_THREADS) void resample_windows_kernel(const RsWin* __restrict__ wins, const float* __restrict__ tab, void* out, int orig,
                                                                      int new_, int width, int K, int G, int fmt) {
    extern __shared__ float smem[];                  // [span] input words, then (TAB_LDS) [K new] table words: sized by the launch, not by the limits
    const RsWin w = wins[blockIdx.y];
    if (w.count <= 0) return;
    const int F = G * RS_R;
    float* xs = smem;
    float* ts = smem + F * orig + 2 * width;
    const long long jlo = w.j0, jhi = w.j0 + w.count;
    const long long fa = (jlo / new_ / F + blockIdx.x) * F;          // first frame of this tile
    if (fa > (jhi - 1) / new_) return;
    const int span = F * orig + 2 * width;
    const long long a0 = fa * orig - width;
    for (int s = threadIdx.x; s < span; s += RS_THREADS) {
        const long long a = a0 + s, r = a - w.src0;
        const bool in = a >= 0 && (w.total < 0 || a < w.total) && r >= 0 && r < w.src_n;
        xs[s] = in ? w.src[r] : 0.f;
    }
    if (TAB_LDS)
        for (int i = threadIdx.x; i < K * new_; i += RS_THREADS) ts[i] = tab[i];
    __syncthreads();
    const float* tb = TAB_LDS ? ts : tab;
    const int PH = (new_ + RP - 1) / RP;             // a thread owns phases ph + q PH, q < RP (the last may not exist: computed on phase ph, not stored)
    const int items = PH * G, rs = G * orig;
    for (int it = threadIdx.x; it < items; it += RS_THREADS) {
        const int ph = it % PH, g = it / PH;
        const float* xb = xs + g * orig;
        int pc[RP];
        float acc[RP][RS_R];
#pragma unroll
        for (int q = 0; q < RP; ++q) {
            pc[q] = ph + q * PH < new_ ? ph + q * PH : ph;
#pragma unroll
            for (int r = 0; r < RS_R; ++r) acc[q][r] = 0.f;
        }
#pragma unroll 2
        for (int k = 0; k < K; ++k) {
            float h[RP], x[RS_R];
#pragma unroll
            for (int q = 0; q < RP; ++q) h[q] = tb[(size_t)k * new_ + pc[q]];
#pragma unroll
            for (int r = 0; r < RS_R; ++r) x[r] = xb[r * rs + k];
#pragma unroll
            for (int q = 0; q < RP; ++q)
#pragma unroll
                for (int r = 0; r < RS_R; ++r) acc[q][r] = fmaf(h[q], x[r], acc[q][r]);
        }
#pragma unroll
        for (int q = 0; q < RP; ++q) {
            if (ph + q * PH >= new_) continue;
#pragma unroll
            for (int r = 0; r < RS_R; ++r) {
                const long long j = (fa + g + (long long)r * G) * new_ + pc[q];
                if (j < jlo || j >= jhi) continue;
                const size_t dst = (size_t)(w.out_off + (j - jlo));
                if (fmt == 1) ((short*)out)[dst] = (short)rintf(fminf(fmaxf(acc[q][r], -1.f), 1.f) * 32767.f);
                else ((float*)out)[dst] = acc[q][r];
            }
        }
    }
}

// ---- host-only geometry ---------------------------------------------------------------------------------------------------------------
static inline long long floor_div(long long a, long long b) { long long q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }

extern "C" int64_t ctts_resample_out_total(int orig, int new_, int64_t n) {
    if (orig < 1 || new_ < 1 || n <= 0) return 0;
    return ((long long)new_ * n + orig - 1) / orig;
}

extern "C" int64_t ctts_resample_settled(int orig, int new_, int width, int64_t S, int finished, int64_t n) {
    if (orig < 1 || new_ < 1) return 0;
    if (finished) return ctts_resample_out_total(orig, new_, n);
    const long long f = floor_div((long long)S - width, orig);
    return (long long)new_ * (f > 0 ? f : 0);
}

extern "C" int ctts_resample_in_range(int orig, int new_, int width, int64_t j0, int64_t j1, int64_t* out2) {
    if (!out2 || orig < 1 || new_ < 1 || width < 0 || j0 < 0) { ctts_set_error("resample_in_range: bad argument"); return 1; }
    out2[0] = out2[1] = 0;
    if (j1 <= j0) return 0;
    out2[0] = (j0 / new_) * orig - width;
    out2[1] = ((j1 - 1) / new_) * orig + orig + width;
    return 0;
}

// ---- the handle -------------------------------------------------------------------------------------------------------------------------
extern "C" int ctts_resampler_create(int orig, int new_, int width, const float* kernels_host, ctts_resampler** out) {
    if (!kernels_host || !out) { ctts_set_error("resampler_create: null argument"); return 1; }
    if (orig < 1 || new_ < 1 || width < 1) { ctts_set_error("resampler_create: orig : new = %d : %d, width = %d (all at least 1)", orig, new_, width); return 1; }
    const long long K = 2LL * width + orig;
    if (K > CTTS_RESAMPLE_MAX_TAPS) {
        ctts_set_error("resampler_create: the rate pair %d : %d needs %lld taps per output sample; the kernel serves at most %d", orig, new_, K, CTTS_RESAMPLE_MAX_TAPS);
        return 1;
    }
    if ((unsigned long long)K * new_ * 4 > CTTS_RESAMPLE_MAX_TABLE_BYTES) {
        ctts_set_error("resampler_create: the rate pair %d : %d needs a filter table of %lld bytes; the kernel serves at most %u", orig, new_, K * new_ * 4,
                       (unsigned)CTTS_RESAMPLE_MAX_TABLE_BYTES);
        return 1;
    }
    ctts_resampler* h = new ctts_resampler();
    h->orig = orig; h->new_ = new_; h->width = width; h->K = (int)K;
    // frame groups per tile: about RS_ITEMS (phase, group) items, and the input span of RS_R G frames must fit xs (G = 1 always does: RS_R K <= RS_XS)
    const int PH = new_ == 1 ? 1 : (new_ + 1) / 2;                  // phase pairs: the kernel's RP = 2 but for new = 1
    int G = RS_ITEMS / PH > 1 ? RS_ITEMS / PH : 1;
    const int fit = (RS_XS - 2 * width) / (RS_R * orig);
    if (G > fit) G = fit > 1 ? fit : 1;
    h->G = G;
    std::vector<float> t((size_t)K * new_);
    for (int p = 0; p < new_; ++p)
        for (int k = 0; k < K; ++k) t[(size_t)k * new_ + p] = kernels_host[(size_t)p * K + k];
    hipError_t e = hipMalloc((void**)&h->d_tab, t.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(h->d_tab, t.data(), t.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_win, RS_TAB_BYTES);
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->pin, 4 * RS_TAB_BYTES, hipHostMallocDefault);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&h->pin_ev[i], hipEventDisableTiming);
    if (e != hipSuccess) {
        ctts_set_error("resampler_create: %s", hipGetErrorString(e));
        ctts_resampler_destroy(h);
        return 1;
    }
    *out = h;
    return 0;
}

extern "C" int ctts_resampler_tile_frames(const ctts_resampler* h) { return h ? h->G * RS_R : 0; }

extern "C" void ctts_resampler_destroy(ctts_resampler* h) {
    if (!h) return;
    for (int i = 0; i < 4; ++i)
        if (h->pin_ev[i]) (void)hipEventDestroy(h->pin_ev[i]);
    if (h->pin) (void)hipHostFree(h->pin);
    if (h->d_win) (void)hipFree(h->d_win);
    if (h->d_tab) (void)hipFree(h->d_tab);
    delete h;
}

extern "C" int ctts_resample_windows(ctts_resampler* h, const float* const* src, const int64_t* src0, const int32_t* src_n, const int64_t* total,
                                     const int64_t* j0, const int32_t* count, int B, void* out, const int64_t* out_off, int fmt, void* stream) {
    if (!h || !src || !src0 || !src_n || !total || !j0 || !count || !out_off) { ctts_set_error("resample_windows: null argument"); return 1; }
    if (B < 1 || B > CTTS_RESAMPLE_MAX_WINDOWS) { ctts_set_error("resample_windows: B=%d outside [1, %d]", B, CTTS_RESAMPLE_MAX_WINDOWS); return 1; }
    if (fmt != 0 && fmt != 1) { ctts_set_error("resample_windows: fmt=%d (0 = float32, 1 = int16 PCM)", fmt); return 1; }
    CTTS_RANGE("ctts_resample_windows");
    const int orig = h->orig, new_ = h->new_, width = h->width, F = h->G * RS_R;
    // every check before the launch: a refused call writes nothing
    long long tiles = 0;
    for (int u = 0; u < B; ++u) {
        if (count[u] < 0 || j0[u] < 0 || src0[u] < 0 || src_n[u] < 0 || out_off[u] < 0 || total[u] < -1) {
            ctts_set_error("resample_windows: window %d: negative j0, count, src0, src_n or out_off, or a total below -1", u);
            return 1;
        }
        if (count[u] == 0) continue;
        const long long j1 = (long long)j0[u] + count[u];
        if (total[u] >= 0 && j1 > ctts_resample_out_total(orig, new_, total[u])) {
            ctts_set_error("resample_windows: window %d: outputs [%lld, %lld) lie outside the %lld outputs of its %lld-sample waveform", u, (long long)j0[u], j1,
                           (long long)ctts_resample_out_total(orig, new_, total[u]), (long long)total[u]);
            return 1;
        }
        long long lo = (j0[u] / new_) * orig - width, hi = ((j1 - 1) / new_) * orig + orig + width;
        if (lo < 0) lo = 0;
        if (total[u] >= 0 && hi > total[u]) hi = total[u];
        const long long b0 = src0[u], b1 = (long long)src0[u] + src_n[u];
        if (hi > lo && (lo < b0 || hi > b1)) {
            ctts_set_error("resample_windows: window %d: outputs [%lld, %lld) read input samples [%lld, %lld), its buffer holds [%lld, %lld)%s", u, (long long)j0[u],
                           j1, lo, hi, b0, b1, total[u] < 0 ? " (total = -1: the waveform's end is not known, every right tap must be in the buffer)" : "");
            return 1;
        }
        if (hi > lo && !src[u]) { ctts_set_error("resample_windows: window %d has no input", u); return 1; }
        const long long t = (j1 - 1) / new_ / F - j0[u] / new_ / F + 1;
        tiles = t > tiles ? t : tiles;
    }
    if (tiles == 0) return 0;                            // nothing to store
    if (!out) { ctts_set_error("resample_windows: null output"); return 1; }
    if (tiles > 0x7fffffffLL) { ctts_set_error("resample_windows: a window of %lld tiles", tiles); return 1; }
    hipStream_t s = (hipStream_t)stream;
    // the windows, staged in a pinned ring slot (a slot is reused only after its copy has run)
    const int slot = h->pin_next++ % 4;
    if (h->pin_used[slot]) CTTS_HIP_CHECK(hipEventSynchronize(h->pin_ev[slot]));
    RsWin* W = (RsWin*)(h->pin + (size_t)slot * RS_TAB_BYTES);
    for (int u = 0; u < B; ++u) W[u] = {src[u], (long long)src0[u], (long long)total[u], (long long)j0[u], (long long)out_off[u], src_n[u], count[u]};
    CTTS_HIP_CHECK(hipMemcpyAsync(h->d_win, W, (size_t)B * sizeof(RsWin), hipMemcpyHostToDevice, s));
    CTTS_HIP_CHECK(hipEventRecord(h->pin_ev[slot], s));
    h->pin_used[slot] = true;
    const dim3 grid((unsigned)tiles, (unsigned)B);
    const size_t span = (size_t)F * orig + 2 * width, tab = (size_t)h->K * new_;            // span <= RS_XS by the choice of G
    const size_t lds = (span + (tab <= RS_TS ? tab : 0)) * 4;
    auto kern = tab <= RS_TS ? (new_ == 1 ? resample_windows_kernel<true, 1> : resample_windows_kernel<true, 2>)
                             : (new_ == 1 ? resample_windows_kernel<false, 1> : resample_windows_kernel<false, 2>);
    hipLaunchKernelGGL(kern, grid, dim3(RS_THREADS), lds, s, (const RsWin*)h->d_win, (const float*)h->d_tab, out, orig, new_, width, h->K, h->G, fmt);
    CTTS_HIP_CHECK(hipGetLastError());
    return 0;
}
