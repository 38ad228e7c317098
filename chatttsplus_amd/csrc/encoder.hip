// Zero-shot speaker path on gfx950: waveform -> log-mel -> DVAE encoder -> GFSQ codes (audio-prompt tokens).
//
// Reference arithmetic:
//   ChatTTSPlusPipeline.sample_audio_speaker      pipelines/chattts_plus_pipeline.py:279-284 (called from :486-499)
//   DVAE.forward(mode="encode")                   models/dvae.py:263-270
//   MelSpectrogramFeatures                        dvae.py:171-199  (third-party torchaudio MelSpectrogram: parity unpinned)
//   downsample_conv (k3 + GELU, k4 stride 2 + GELU), encoder = DVAEDecoder(512 -> 1024, hidden 256)   dvae.py:224-231,130-168
//   GFSQ.forward                                  dvae.py:94-126   (third-party vector_quantize_pytorch 1.17.8: parity unpinned)
//
// Same lowering as vocoder.hip (conv_gemm.h): channels-last rows, every Conv1d is a GEMM over overlapping row windows of a
// zero-guarded buffer.  Two more instances of that trick:
//   * the STFT: frame f is the 1024-sample window starting at sample 256 f of the reflect-padded signal -> A = padded signal,
//     row stride 256 (the hop), K = 1024, against a windowed real-DFT basis [cos | -sin]: no frame buffer;
//   * the stride-2 k4 conv: output t reads input rows 2t-1 .. 2t+2 -> row stride 2 C, K = 4 C.
#include <map>
#include <string>

#include "conv_gemm.h"
#include "roctx_range.h"

struct EncConvNext { float *dw_w, *dw_b, *ln_w, *ln_b, *w1, *b1, *w2, *b2, *gamma; };

// one utterance of a ctts_dvae_encode_batch call; the call's device table is [EncUtt x B][Fs x B][Ts x B], uploaded once
struct EncUtt { const float* wav; int* ids; float *mel, *feat; int n, F, T, pad; };
#define ENC_TAB_BYTES ((size_t)CTTS_ENC_MAX_BATCH * (sizeof(EncUtt) + 8))
#define ENC_BATCH_WS 4

struct ctts_enc {
    ctts_enc_cfg cfg;
    std::map<std::string, std::vector<float>> host;
    bool finalized = false;
    std::vector<void*> allocs;
    float *basis, *fbw, *coef, *ds0_w, *ds0_b, *ds2_w, *ds2_b, *ci0_w, *ci0_b, *ci2_w, *ci2_b, *co_w, *pin_w, *pin_b;
    std::vector<EncConvNext> blocks;
    float *xp, *spec, *mag, *melcl, *d1, *x2, *b128, *y, *ln, *mid, *feat;
    int* d_T;
    int Fmax, spec_ld, mag_ld, mel_ld;
    // batch path (ctts_dvae_encode_batch): `ws` is the workspace set it chunks a batch into -- the single-clip buffers above until a
    // call needs more, then a set ENC_BATCH_WS times as large, allocated once; the per-call tables go through a pinned ring
    struct Ws { float *xp, *spec, *mag, *melcl, *d1, *x2, *b128, *y, *ln, *mid, *feat; size_t n_xp, rowsF, rowsD1, rowsT; } ws = {};
    bool ws_big = false;
    char *pin = nullptr, *d_tab = nullptr;
    hipEvent_t pin_ev[4] = {};
    bool pin_used[4] = {};
    int pin_next = 0;
};

static int ealloc(ctts_enc* h, float** p, size_t n) {
    CTTS_HIP_CHECK(hipMalloc((void**)p, n * 4));
    CTTS_HIP_CHECK(hipMemset(*p, 0, n * 4));
    h->allocs.push_back(*p);
    return 0;
}
static int eupload(ctts_enc* h, float** p, const std::vector<float>& v) {
    if (ealloc(h, p, v.size())) return 1;
    CTTS_HIP_CHECK(hipMemcpy(*p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    return 0;
}
static const std::vector<float>* eneed(ctts_enc* h, const std::string& k, size_t n) {
    auto it = h->host.find(k);
    if (it == h->host.end()) { ctts_set_error("missing weight %s", k.c_str()); return nullptr; }
    if (it->second.size() != n) { ctts_set_error("weight %s has %zu elements, expected %zu", k.c_str(), it->second.size(), n); return nullptr; }
    return &it->second;
}

// reflect padding of torch.stft(center=True, pad_mode="reflect"): xp[i] = x[reflect(i - n_fft/2)]
__global__ void reflect_pad_kernel(const float* x, float* xp, int n, int half, int total) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int j = i - half;
    if (j < 0) j = -j;
    if (j >= n) j = 2 * (n - 1) - j;
    xp[i] = (j >= 0 && j < n) ? x[j] : 0.f;
}

// |X_k| from the [re | im] GEMM output; columns nb..ld-1 are zero padding of the mel GEMM's K
__global__ void magnitude_kernel(const float* spec, float* mag, int F, int nb, int lds, int ldm) {
    const int f = blockIdx.x;
    for (int k = threadIdx.x; k < ldm; k += blockDim.x) {
        float v = 0.f;
        if (k < nb) {
            const float re = spec[(size_t)f * lds + k], im = spec[(size_t)f * lds + nb + k];
            v = sqrtf(re * re + im * im);
        }
        mag[(size_t)f * ldm + k] = v;
    }
}

// mel [F][ld] channels-last -> API layout [n_mels][F] (test hook output)
__global__ void mel_out_kernel(const float* melcl, float* mel, int F, int n_mels, int ld) {
    const int f = blockIdx.x, c = threadIdx.x;
    if (c < n_mels) mel[(size_t)c * F + f] = melcl[(size_t)f * ld + c];
}

// GFSQ.forward (dvae.py:94-126) -> GroupedResidualFSQ: group g = channels [g*per, (g+1)*per); project_in to 4 dims; two
// residual FSQ layers, levels 5^4: code = rint(tanh(z) * 2.002) / 2, index = sum (2 code + 2) * 5^j, scale_r = 4^-r.
// One wave per (frame, group).
// Non-finite audio: a NaN or +-inf sample makes every mel frame whose window covers it NaN (the STFT row holds NaN or inf, the filterbank's zeros turn inf into NaN,
// and the mel epilogue's clip keeps NaN as torch.clip does); the conv stack spreads it over its receptive field.  A (frame, group) whose projected z is not
// finite gets id -1 in all R rows -- never a value in [0, 625) -- so that the caller can refuse the clip.  Finite clips are untouched.
__device__ inline bool gfsq_nonfinite(const float (&z)[4]) {
    return !(__builtin_isfinite(z[0]) && __builtin_isfinite(z[1]) && __builtin_isfinite(z[2]) && __builtin_isfinite(z[3]));
}
__global__ __launch_bounds__(64) void gfsq_kernel(const float* feat, const float* w, const float* b, int* ids, int T, int per, int ld, int R, int pre_bound) {
    const int t = blockIdx.x, g = blockIdx.y, lane = threadIdx.x;
    const float* x = feat + (size_t)t * ld + (size_t)g * per;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < per; c += 64) {
        const float xv = x[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] += w[((size_t)g * 4 + j) * per + c] * xv;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = wave_sum(z[j]) + b[g * 4 + j];
    if (lane != 0) return;
    if (gfsq_nonfinite(z)) {                                       // rintf(NaN) cast to int would be a plausible id
        for (int r = 0; r < R; ++r) ids[(size_t)(g * R + r) * T + t] = -1;
        return;
    }
    const float half_l = 2.002f;                                   // (levels - 1) * (1 + 1e-3) / 2 in fp32
    float res[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) res[j] = pre_bound ? tanhf(z[j]) * half_l : z[j];
    float scale = 1.0f;
    for (int r = 0; r < R; ++r) {
        int idx = 0, basis = 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float q = rintf(tanhf(res[j] / scale) * half_l);  // torch.round: half to even
            const float code = q / 2.0f;
            idx += (int)(code * 2.0f + 2.0f) * basis;
            basis *= 5;
            res[j] -= code * scale;
        }
        ids[(size_t)(g * R + r) * T + t] = idx;
        scale *= 0.25f;                                            // (levels - 1) ** -(r + 1)
    }
}

// ---- the same kernels keyed by utterance (ctts_dvae_encode_batch): blockIdx.y (gfsq: z) = utterance of the chunk, its sizes and
// pointers come from the EncUtt table, its workspace region from a batch stride.  Arithmetic term for term that of the kernels above.
__global__ void reflect_pad_batch_kernel(const EncUtt* U, float* xp, long sxp, int half) {
    const EncUtt u = U[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x, n = u.n;
    if (i >= n + 2 * half) return;
    int j = i - half;
    if (j < 0) j = -j;
    if (j >= n) j = 2 * (n - 1) - j;
    xp[(size_t)blockIdx.y * sxp + i] = (j >= 0 && j < n) ? u.wav[j] : 0.f;
}

__global__ void magnitude_batch_kernel(const float* spec, float* mag, const int* Fs, long ss, long sm, int nb, int lds, int ldm) {
    const int f = blockIdx.x;
    if (f >= Fs[blockIdx.y]) return;
    spec += (size_t)blockIdx.y * ss; mag += (size_t)blockIdx.y * sm;
    for (int k = threadIdx.x; k < ldm; k += blockDim.x) {
        float v = 0.f;
        if (k < nb) {
            const float re = spec[(size_t)f * lds + k], im = spec[(size_t)f * lds + nb + k];
            v = sqrtf(re * re + im * im);
        }
        mag[(size_t)f * ldm + k] = v;
    }
}

// zeroes, for every utterance of the chunk, the guard rows the single-clip path clears with its memsets: mel image rows 0 and F + 1,
// d1 rows 0 and F + 1 .. F + 3, x2 and b128 rows 0 and T + 1 (a longer clip of an earlier call or chunk may have left data there)
__global__ void guard_rows_batch_kernel(const EncUtt* U, float* melcl, float* d1, float* x2, float* b128, long smel, long sd1, long sx2, long sb,
                                        int mel_ld, int D, int BN) {
    const EncUtt u = U[blockIdx.x];
    const size_t z = blockIdx.x;
    float *m = melcl + z * smel, *d = d1 + z * sd1, *x = x2 + z * sx2, *b = b128 + z * sb;
    for (int c = threadIdx.x; c < mel_ld; c += blockDim.x) { m[c] = 0.f; m[(size_t)(u.F + 1) * mel_ld + c] = 0.f; }
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        d[c] = 0.f;
        for (int r = 1; r <= 3; ++r) d[(size_t)(u.F + r) * D + c] = 0.f;
        x[c] = 0.f; x[(size_t)(u.T + 1) * D + c] = 0.f;
    }
    for (int c = threadIdx.x; c < BN; c += blockDim.x) { b[c] = 0.f; b[(size_t)(u.T + 1) * BN + c] = 0.f; }
}

// test hooks: mel image -> [n_mels][F_u], encoder output -> [T_u][OD]; an utterance without the hook is skipped
__global__ void mel_out_batch_kernel(const EncUtt* U, const float* melcl, long smel, int n_mels, int ld) {
    const EncUtt u = U[blockIdx.y];
    const int f = blockIdx.x, c = threadIdx.x;
    if (!u.mel || f >= u.F || c >= n_mels) return;
    u.mel[(size_t)c * u.F + f] = melcl[(size_t)blockIdx.y * smel + (size_t)(f + 1) * ld + c];
}
__global__ void feat_out_batch_kernel(const EncUtt* U, const float* feat, long sf, int OD) {
    const EncUtt u = U[blockIdx.y];
    const int t = blockIdx.x;
    if (!u.feat || t >= u.T) return;
    for (int c = threadIdx.x; c < OD; c += blockDim.x) u.feat[(size_t)t * OD + c] = feat[(size_t)blockIdx.y * sf + (size_t)t * OD + c];
}

__global__ __launch_bounds__(64) void gfsq_batch_kernel(const EncUtt* U, const float* feat, long sf, const float* w, const float* b, int per, int ld, int R, int pre_bound) {
    const EncUtt u = U[blockIdx.z];
    const int t = blockIdx.x, g = blockIdx.y, lane = threadIdx.x, T = u.T;
    if (t >= T) return;
    const float* x = feat + (size_t)blockIdx.z * sf + (size_t)t * ld + (size_t)g * per;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < per; c += 64) {
        const float xv = x[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] += w[((size_t)g * 4 + j) * per + c] * xv;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = wave_sum(z[j]) + b[g * 4 + j];
    if (lane != 0) return;
    if (gfsq_nonfinite(z)) {
        for (int r = 0; r < R; ++r) u.ids[(size_t)(g * R + r) * T + t] = -1;
        return;
    }
    const float half_l = 2.002f;
    float res[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) res[j] = pre_bound ? tanhf(z[j]) * half_l : z[j];
    float scale = 1.0f;
    for (int r = 0; r < R; ++r) {
        int idx = 0, basis = 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float q = rintf(tanhf(res[j] / scale) * half_l);
            const float code = q / 2.0f;
            idx += (int)(code * 2.0f + 2.0f) * basis;
            basis *= 5;
            res[j] -= code * scale;
        }
        u.ids[(size_t)(g * R + r) * T + t] = idx;
        scale *= 0.25f;
    }
}

extern "C" int ctts_enc_create(const ctts_enc_cfg* c, ctts_enc** out) {
    if (!c || !out) { ctts_set_error("null argument"); return 1; }
    if (c->dim != 512 || c->enc_hidden != 256 || c->enc_bn % 64 || c->enc_odim % 64 || c->n_fft != 1024 || c->hop != 256 || c->n_mels > 112 ||
        c->vq_groups < 1 || c->vq_groups > 8 || c->enc_odim % c->vq_groups || c->vq_residuals < 1 || c->vq_residuals > 8 || c->max_samples < c->n_fft) {
        ctts_set_error("unsupported encoder configuration");
        return 1;
    }
    ctts_enc* h = new ctts_enc();
    h->cfg = *c;
    *out = h;
    return 0;
}
extern "C" void ctts_enc_destroy(ctts_enc* h) {
    if (!h) return;
    if (h->pin) (void)hipHostFree(h->pin);
    for (hipEvent_t e : h->pin_ev) if (e) (void)hipEventDestroy(e);
    for (void* p : h->allocs) (void)hipFree(p);
    delete h;
}
extern "C" int ctts_enc_set_weight(ctts_enc* h, const char* name, const float* data, size_t numel) {
    if (!h || !name || !data) { ctts_set_error("null argument"); return 1; }
    if (h->finalized) { ctts_set_error("weights already finalized"); return 1; }
    h->host[std::string(name)].assign(data, data + numel);
    return 0;
}

extern "C" int ctts_enc_finalize(ctts_enc* h) {
    if (!h) { ctts_set_error("null handle"); return 1; }
    if (h->finalized) return 0;
    const ctts_enc_cfg& c = h->cfg;
    const int NM = c.n_mels, D = c.dim, HD = c.enc_hidden, BN = c.enc_bn, OD = c.enc_odim, N = c.n_fft, NB = N / 2 + 1;
    h->mel_ld = 112; h->mag_ld = (NB + 15) / 16 * 16; h->spec_ld = r64(2 * NB);
    // windowed forward real-DFT basis rows: k < NB: w[n] cos(2 pi k n / N);  NB + k: -w[n] sin(2 pi k n / N)
    const std::vector<float>* win = eneed(h, "mel.window", N);
    const std::vector<float>* fb = eneed(h, "mel.fb", (size_t)NB * NM);
    if (!win || !fb) return 1;
    {
        std::vector<float> B((size_t)h->spec_ld * N, 0.f);
        for (int k = 0; k < NB; ++k)
            for (int n = 0; n < N; ++n) {
                const double ang = 2.0 * M_PI * (double)((long long)k * n % N) / N;
                B[(size_t)k * N + n] = (float)((*win)[n] * cos(ang));
                B[(size_t)(NB + k) * N + n] = (float)(-(double)(*win)[n] * sin(ang));
            }
        if (eupload(h, &h->basis, B)) return 1;
        std::vector<float> W((size_t)r64(NM) * h->mag_ld, 0.f);       // mel filterbank transposed: [n_mels][n_freqs]
        for (int k = 0; k < NB; ++k)
            for (int m = 0; m < NM; ++m) W[(size_t)m * h->mag_ld + k] = (*fb)[(size_t)k * NM + m];
        if (eupload(h, &h->fbw, W)) return 1;
    }
    const std::vector<float>*w, *b;
    w = eneed(h, "coef", NM);
    if (!w || eupload(h, &h->coef, *w)) return 1;
    w = eneed(h, "downsample_conv.0.weight", (size_t)D * NM * 3); b = eneed(h, "downsample_conv.0.bias", D);
    if (!w || !b || eupload(h, &h->ds0_w, conv_to_gemm(*w, D, NM, 3, h->mel_ld, r64(D))) || eupload(h, &h->ds0_b, *b)) return 1;
    w = eneed(h, "downsample_conv.2.weight", (size_t)D * D * 4); b = eneed(h, "downsample_conv.2.bias", D);
    if (!w || !b || eupload(h, &h->ds2_w, conv_to_gemm(*w, D, D, 4, D, r64(D))) || eupload(h, &h->ds2_b, *b)) return 1;
    w = eneed(h, "encoder.conv_in.0.weight", (size_t)BN * D * 3); b = eneed(h, "encoder.conv_in.0.bias", BN);
    if (!w || !b || eupload(h, &h->ci0_w, conv_to_gemm(*w, BN, D, 3, D, r64(BN))) || eupload(h, &h->ci0_b, *b)) return 1;
    w = eneed(h, "encoder.conv_in.2.weight", (size_t)HD * BN * 3); b = eneed(h, "encoder.conv_in.2.bias", HD);
    if (!w || !b || eupload(h, &h->ci2_w, conv_to_gemm(*w, HD, BN, 3, BN, r64(HD))) || eupload(h, &h->ci2_b, *b)) return 1;
    h->blocks.resize(c.enc_layers);
    for (int i = 0; i < c.enc_layers; ++i) {
        const std::string p = "encoder.decoder_block." + std::to_string(i) + ".";
        const int inter = HD * 4;
        const std::vector<float>*dw = eneed(h, p + "dwconv.weight", (size_t)HD * 7), *db = eneed(h, p + "dwconv.bias", HD),
                                *lw = eneed(h, p + "norm.weight", HD), *lb = eneed(h, p + "norm.bias", HD),
                                *w1 = eneed(h, p + "pwconv1.weight", (size_t)inter * HD), *b1 = eneed(h, p + "pwconv1.bias", inter),
                                *w2 = eneed(h, p + "pwconv2.weight", (size_t)HD * inter), *b2 = eneed(h, p + "pwconv2.bias", HD),
                                *g = eneed(h, p + "gamma", HD);
        if (!dw || !db || !lw || !lb || !w1 || !b1 || !w2 || !b2 || !g) return 1;
        EncConvNext& cb = h->blocks[i];
        if (eupload(h, &cb.dw_w, *dw) || eupload(h, &cb.dw_b, *db) || eupload(h, &cb.ln_w, *lw) || eupload(h, &cb.ln_b, *lb) ||
            eupload(h, &cb.w1, *w1) || eupload(h, &cb.b1, *b1) || eupload(h, &cb.w2, *w2) || eupload(h, &cb.b2, *b2) || eupload(h, &cb.gamma, *g))
            return 1;
    }
    w = eneed(h, "encoder.conv_out.weight", (size_t)OD * HD);
    if (!w || eupload(h, &h->co_w, pad_rows(*w, OD, HD, r64(OD)))) return 1;
    {
        const int G = c.vq_groups, per = OD / G;
        std::vector<float> pw((size_t)G * 4 * per), pb((size_t)G * 4);
        for (int g = 0; g < G; ++g) {
            const std::string p = "vq_layer.quantizer.rvqs." + std::to_string(g) + ".project_in.";
            w = eneed(h, p + "weight", (size_t)4 * per); b = eneed(h, p + "bias", 4);
            if (!w || !b) return 1;
            memcpy(pw.data() + (size_t)g * 4 * per, w->data(), (size_t)4 * per * 4);
            memcpy(pb.data() + (size_t)g * 4, b->data(), 16);
        }
        if (eupload(h, &h->pin_w, pw) || eupload(h, &h->pin_b, pb)) return 1;
    }
    // workspaces: F = 1 + n / hop frames, T = (F - 2) / 2 + 1 codes; rows padded so that every 64-row GEMM tile stays in bounds
    const int Fmax = 1 + c.max_samples / c.hop;
    h->Fmax = Fmax;
    const size_t Fp = r64(Fmax) + 64 + 8, Tp = r64(Fmax / 2 + 1) + 64 + 8;
    if (ealloc(h, &h->xp, (size_t)(r64(Fmax) + 64) * c.hop + N) || ealloc(h, &h->spec, Fp * h->spec_ld) || ealloc(h, &h->mag, Fp * h->mag_ld) ||
        ealloc(h, &h->melcl, Fp * h->mel_ld) || ealloc(h, &h->d1, (Fp + 136) * D) || ealloc(h, &h->x2, Tp * D) || ealloc(h, &h->b128, Tp * BN) ||
        ealloc(h, &h->y, Tp * HD) || ealloc(h, &h->ln, Tp * HD) || ealloc(h, &h->mid, Tp * HD * 4) || ealloc(h, &h->feat, Tp * OD))
        return 1;
    CTTS_HIP_CHECK(hipMalloc((void**)&h->d_T, 16));
    h->allocs.push_back(h->d_T);
    h->ws = {h->xp, h->spec, h->mag, h->melcl, h->d1, h->x2, h->b128, h->y, h->ln, h->mid, h->feat, (size_t)(r64(Fmax) + 64) * c.hop + N, Fp, Fp + 136, Tp};
    CTTS_HIP_CHECK(hipMalloc((void**)&h->d_tab, ENC_TAB_BYTES));
    h->allocs.push_back(h->d_tab);
    CTTS_HIP_CHECK(hipHostMalloc((void**)&h->pin, 4 * ENC_TAB_BYTES, hipHostMallocDefault));
    for (hipEvent_t& e : h->pin_ev) CTTS_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    h->host.clear();
    h->finalized = true;
    return 0;
}

extern "C" int ctts_dvae_encode(ctts_enc* h, const float* wav, int n_samples, int32_t* ids, float* mel_out, float* feat_out, void* stream) {
    if (!h || !h->finalized || !wav || !ids) { ctts_set_error("dvae_encode: bad argument"); return 1; }
    CTTS_RANGE("ctts_dvae_encode");
    const ctts_enc_cfg& c = h->cfg;
    const int N = c.n_fft, hop = c.hop, NB = N / 2 + 1, D = c.dim, HD = c.enc_hidden, BN = c.enc_bn, OD = c.enc_odim;
    if (n_samples <= N / 2 || n_samples > c.max_samples) {        // reflect padding needs n > n_fft / 2 (torch.stft raises otherwise)
        ctts_set_error("dvae_encode: %d samples outside (%d, %d]", n_samples, N / 2, c.max_samples);
        return 1;
    }
    const int F = 1 + n_samples / hop, T = (F - 2) / 2 + 1;
    if (F < 2) { ctts_set_error("dvae_encode: too short"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    // 1. reflect-padded signal (rows of the STFT GEMM overlap: frame f = xp[256 f .. 256 f + 1023])
    const int total = n_samples + N;
    hipLaunchKernelGGL(reflect_pad_kernel, dim3((total + 255) / 256), dim3(256), 0, s, wav, h->xp, n_samples, N / 2, total);
    CTTS_HIP_CHECK(hipGetLastError());
    GemmF32Args g = {};
    g.A = h->xp; g.lda = hop; g.W = h->basis; g.ldw = N; g.C = h->spec; g.ldc = h->spec_ld; g.M = F; g.N = 2 * NB; g.K = N;
    if (launch_gemm_f32(EP_NONE, g, 1, s)) return 1;                                       // torch.stft (dvae.py:186-193)
    hipLaunchKernelGGL(magnitude_kernel, dim3(F), dim3(256), 0, s, h->spec, h->mag, F, NB, h->spec_ld, h->mag_ld);   // power = 1
    CTTS_HIP_CHECK(hipGetLastError());
    // zero guard rows of this call's conv inputs (a longer previous call may have left data there)
    CTTS_HIP_CHECK(hipMemsetAsync(h->melcl, 0, (size_t)h->mel_ld * 4, s));
    CTTS_HIP_CHECK(hipMemsetAsync(h->melcl + (size_t)(F + 1) * h->mel_ld, 0, (size_t)h->mel_ld * 4, s));
    CTTS_HIP_CHECK(hipMemsetAsync(h->d1, 0, (size_t)D * 4, s));
    CTTS_HIP_CHECK(hipMemsetAsync(h->d1 + (size_t)(F + 1) * D, 0, (size_t)3 * D * 4, s));
    CTTS_HIP_CHECK(hipMemsetAsync(h->x2, 0, (size_t)D * 4, s));
    CTTS_HIP_CHECK(hipMemsetAsync(h->x2 + (size_t)(T + 1) * D, 0, (size_t)D * 4, s));
    CTTS_HIP_CHECK(hipMemsetAsync(h->b128, 0, (size_t)BN * 4, s));
    CTTS_HIP_CHECK(hipMemsetAsync(h->b128 + (size_t)(T + 1) * BN, 0, (size_t)BN * 4, s));
    CTTS_HIP_CHECK(hipMemcpyAsync(h->d_T, &T, 4, hipMemcpyHostToDevice, s));               // pageable source: staged before return
    GemmF32Args gm = {};
    gm.A = h->mag; gm.lda = h->mag_ld; gm.W = h->fbw; gm.ldw = h->mag_ld; gm.C = h->melcl + h->mel_ld; gm.ldc = h->mel_ld;
    gm.M = F; gm.N = c.n_mels; gm.K = h->mag_ld; gm.scale = h->coef;
    if (launch_gemm_f32(EP_LOGCLIP_DIV, gm, 1, s)) return 1;                               // MelScale, log(clip), / coef (dvae.py:196-198,264-266)
    if (mel_out) {                                                                         // test hook: log-mel / coef, [n_mels][F]
        hipLaunchKernelGGL(mel_out_kernel, dim3(F), dim3(128), 0, s, h->melcl + h->mel_ld, mel_out, F, c.n_mels, h->mel_ld);
        CTTS_HIP_CHECK(hipGetLastError());
    }
    GemmF32Args g1 = {};
    g1.A = h->melcl; g1.lda = h->mel_ld; g1.W = h->ds0_w; g1.ldw = 3 * h->mel_ld; g1.C = h->d1 + D; g1.ldc = D; g1.M = F; g1.N = D; g1.K = 3 * h->mel_ld;
    g1.bias = h->ds0_b;
    if (launch_gemm_f32(EP_BIAS_GELU, g1, 1, s)) return 1;                                 // downsample_conv.0 k3 p1 + GELU
    GemmF32Args g2 = {};
    g2.A = h->d1; g2.lda = 2 * D; g2.W = h->ds2_w; g2.ldw = 4 * D; g2.C = h->x2 + D; g2.ldc = D; g2.M = T; g2.N = D; g2.K = 4 * D; g2.bias = h->ds2_b;
    if (launch_gemm_f32(EP_BIAS_GELU, g2, 1, s)) return 1;                                 // downsample_conv.2 k4 stride 2 p1 + GELU
    GemmF32Args g3 = {};
    g3.A = h->x2; g3.lda = D; g3.W = h->ci0_w; g3.ldw = 3 * D; g3.C = h->b128 + BN; g3.ldc = BN; g3.M = T; g3.N = BN; g3.K = 3 * D; g3.bias = h->ci0_b;
    if (launch_gemm_f32(EP_BIAS_GELU, g3, 1, s)) return 1;                                 // encoder.conv_in.0 + GELU
    GemmF32Args g4 = {};
    g4.A = h->b128; g4.lda = BN; g4.W = h->ci2_w; g4.ldw = 3 * BN; g4.C = h->y; g4.ldc = HD; g4.M = T; g4.N = HD; g4.K = 3 * BN; g4.bias = h->ci2_b;
    if (launch_gemm_f32(EP_BIAS, g4, 1, s)) return 1;                                      // encoder.conv_in.2
    for (int i = 0; i < c.enc_layers; ++i) {                                               // ConvNeXt, dilation 2 (dvae.py:147-158)
        const EncConvNext& cb = h->blocks[i];
        hipLaunchKernelGGL(dwconv_ln_kernel<4>, dim3((T + 3) / 4, 1), dim3(256), 0, s, h->y, h->ln, cb.dw_w, cb.dw_b, cb.ln_w, cb.ln_b, h->d_T, 0L, 0L, HD, 2, 7);
        CTTS_HIP_CHECK(hipGetLastError());
        GemmF32Args a1 = {};
        a1.A = h->ln; a1.lda = HD; a1.W = cb.w1; a1.ldw = HD; a1.C = h->mid; a1.ldc = HD * 4; a1.M = T; a1.N = HD * 4; a1.K = HD; a1.bias = cb.b1;
        if (launch_gemm_f32(EP_BIAS_GELU, a1, 1, s)) return 1;
        GemmF32Args a2 = {};
        a2.A = h->mid; a2.lda = HD * 4; a2.W = cb.w2; a2.ldw = HD * 4; a2.C = h->y; a2.ldc = HD; a2.M = T; a2.N = HD; a2.K = HD * 4; a2.bias = cb.b2;
        a2.gamma = cb.gamma; a2.resid = h->y; a2.ldr = HD;
        if (launch_gemm_f32(EP_GAMMA_RESID, a2, 1, s)) return 1;
    }
    GemmF32Args g5 = {};
    g5.A = h->y; g5.lda = HD; g5.W = h->co_w; g5.ldw = HD; g5.C = h->feat; g5.ldc = OD; g5.M = T; g5.N = OD; g5.K = HD;
    if (launch_gemm_f32(EP_NONE, g5, 1, s)) return 1;                                      // encoder.conv_out 1x1
    if (feat_out) CTTS_HIP_CHECK(hipMemcpyAsync(feat_out, h->feat, (size_t)T * OD * 4, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(gfsq_kernel, dim3(T, c.vq_groups), dim3(64), 0, s, h->feat, h->pin_w, h->pin_b, (int*)ids, T, OD / c.vq_groups, OD,
                       c.vq_residuals, c.pre_bound);
    CTTS_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- batch ----------------------------------------------------------------------------------------------------------------------------
// Workspace rows one utterance region needs when the longest clip of its chunk has Fc frames: the single-clip formulas of ctts_enc_finalize
// with Fc in place of Fmax (64-row GEMM tiles stay inside the region, guard rows included).
struct EncRegion { size_t n_xp, rowsF, rowsD1, rowsT; };
static EncRegion enc_region(const ctts_enc_cfg& c, int Fc) {
    const size_t Fp = r64(Fc) + 64 + 8;
    return {(size_t)(r64(Fc) + 64) * c.hop + c.n_fft, Fp, Fp + 136, (size_t)r64(Fc / 2 + 1) + 64 + 8};
}
static bool enc_fits(const ctts_enc::Ws& w, const EncRegion& r, size_t nb) {
    return nb * r.n_xp <= w.n_xp && nb * r.rowsF <= w.rowsF && nb * r.rowsD1 <= w.rowsD1 && nb * r.rowsT <= w.rowsT;
}

// one launch sequence for utterances [u0, u0 + nb) of the call's table; Fc / Tc / nmax: the longest of the chunk
static int encode_chunk(ctts_enc* h, int u0, int nb, int Fc, int Tc, int nmax, bool any_mel, bool any_feat, hipStream_t s) {
    const ctts_enc_cfg& c = h->cfg;
    const ctts_enc::Ws& w = h->ws;
    const int N = c.n_fft, hop = c.hop, NB = N / 2 + 1, D = c.dim, HD = c.enc_hidden, BN = c.enc_bn, OD = c.enc_odim;
    const EncRegion r = enc_region(c, Fc);
    const EncUtt* U = (const EncUtt*)h->d_tab + u0;
    const int* Fs = (const int*)(h->d_tab + (size_t)CTTS_ENC_MAX_BATCH * sizeof(EncUtt)) + u0;
    const int* Ts = Fs + CTTS_ENC_MAX_BATCH;
    const long sxp = (long)r.n_xp, sspec = (long)r.rowsF * h->spec_ld, smag = (long)r.rowsF * h->mag_ld, smel = (long)r.rowsF * h->mel_ld,
               sd1 = (long)r.rowsD1 * D, sx2 = (long)r.rowsT * D, sb = (long)r.rowsT * BN, sy = (long)r.rowsT * HD, smid = (long)r.rowsT * HD * 4,
               sfeat = (long)r.rowsT * OD;
    hipLaunchKernelGGL(reflect_pad_batch_kernel, dim3((nmax + N + 255) / 256, nb), dim3(256), 0, s, U, w.xp, sxp, N / 2);
    CTTS_HIP_CHECK(hipGetLastError());
    GemmF32Args g = {};
    g.A = w.xp; g.lda = hop; g.sA = sxp; g.W = h->basis; g.ldw = N; g.C = w.spec; g.ldc = h->spec_ld; g.sC = sspec; g.M = Fc; g.Ms = Fs; g.N = 2 * NB; g.K = N;
    if (launch_gemm_f32(EP_NONE, g, nb, s)) return 1;                                      // torch.stft (dvae.py:186-193)
    hipLaunchKernelGGL(magnitude_batch_kernel, dim3(Fc, nb), dim3(256), 0, s, w.spec, w.mag, Fs, sspec, smag, NB, h->spec_ld, h->mag_ld);
    CTTS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(guard_rows_batch_kernel, dim3(nb), dim3(256), 0, s, U, w.melcl, w.d1, w.x2, w.b128, smel, sd1, sx2, sb, h->mel_ld, D, BN);
    CTTS_HIP_CHECK(hipGetLastError());
    GemmF32Args gm = {};
    gm.A = w.mag; gm.lda = h->mag_ld; gm.sA = smag; gm.W = h->fbw; gm.ldw = h->mag_ld; gm.C = w.melcl + h->mel_ld; gm.ldc = h->mel_ld; gm.sC = smel;
    gm.M = Fc; gm.Ms = Fs; gm.N = c.n_mels; gm.K = h->mag_ld; gm.scale = h->coef;
    if (launch_gemm_f32(EP_LOGCLIP_DIV, gm, nb, s)) return 1;                              // MelScale, log(clip), / coef
    if (any_mel) {
        hipLaunchKernelGGL(mel_out_batch_kernel, dim3(Fc, nb), dim3(128), 0, s, U, w.melcl, smel, c.n_mels, h->mel_ld);
        CTTS_HIP_CHECK(hipGetLastError());
    }
    GemmF32Args g1 = {};
    g1.A = w.melcl; g1.lda = h->mel_ld; g1.sA = smel; g1.W = h->ds0_w; g1.ldw = 3 * h->mel_ld; g1.C = w.d1 + D; g1.ldc = D; g1.sC = sd1;
    g1.M = Fc; g1.Ms = Fs; g1.N = D; g1.K = 3 * h->mel_ld; g1.bias = h->ds0_b;
    if (launch_gemm_f32(EP_BIAS_GELU, g1, nb, s)) return 1;                                // downsample_conv.0 k3 p1 + GELU
    GemmF32Args g2 = {};
    g2.A = w.d1; g2.lda = 2 * D; g2.sA = sd1; g2.W = h->ds2_w; g2.ldw = 4 * D; g2.C = w.x2 + D; g2.ldc = D; g2.sC = sx2;
    g2.M = Tc; g2.Ms = Ts; g2.N = D; g2.K = 4 * D; g2.bias = h->ds2_b;
    if (launch_gemm_f32(EP_BIAS_GELU, g2, nb, s)) return 1;                                // downsample_conv.2 k4 stride 2 p1 + GELU
    GemmF32Args g3 = {};
    g3.A = w.x2; g3.lda = D; g3.sA = sx2; g3.W = h->ci0_w; g3.ldw = 3 * D; g3.C = w.b128 + BN; g3.ldc = BN; g3.sC = sb;
    g3.M = Tc; g3.Ms = Ts; g3.N = BN; g3.K = 3 * D; g3.bias = h->ci0_b;
    if (launch_gemm_f32(EP_BIAS_GELU, g3, nb, s)) return 1;                                // encoder.conv_in.0 + GELU
    GemmF32Args g4 = {};
    g4.A = w.b128; g4.lda = BN; g4.sA = sb; g4.W = h->ci2_w; g4.ldw = 3 * BN; g4.C = w.y; g4.ldc = HD; g4.sC = sy;
    g4.M = Tc; g4.Ms = Ts; g4.N = HD; g4.K = 3 * BN; g4.bias = h->ci2_b;
    if (launch_gemm_f32(EP_BIAS, g4, nb, s)) return 1;                                     // encoder.conv_in.2
    for (int i = 0; i < c.enc_layers; ++i) {                                               // ConvNeXt, dilation 2 (dvae.py:147-158)
        const EncConvNext& cb = h->blocks[i];
        hipLaunchKernelGGL(dwconv_ln_kernel<4>, dim3((Tc + 3) / 4, nb), dim3(256), 0, s, w.y, w.ln, cb.dw_w, cb.dw_b, cb.ln_w, cb.ln_b, Ts, sy, sy, HD, 2, 7);
        CTTS_HIP_CHECK(hipGetLastError());
        GemmF32Args a1 = {};
        a1.A = w.ln; a1.lda = HD; a1.sA = sy; a1.W = cb.w1; a1.ldw = HD; a1.C = w.mid; a1.ldc = HD * 4; a1.sC = smid;
        a1.M = Tc; a1.Ms = Ts; a1.N = HD * 4; a1.K = HD; a1.bias = cb.b1;
        if (launch_gemm_f32(EP_BIAS_GELU, a1, nb, s)) return 1;
        GemmF32Args a2 = {};
        a2.A = w.mid; a2.lda = HD * 4; a2.sA = smid; a2.W = cb.w2; a2.ldw = HD * 4; a2.C = w.y; a2.ldc = HD; a2.sC = sy;
        a2.M = Tc; a2.Ms = Ts; a2.N = HD; a2.K = HD * 4; a2.bias = cb.b2; a2.gamma = cb.gamma; a2.resid = w.y; a2.ldr = HD; a2.sR = sy;
        if (launch_gemm_f32(EP_GAMMA_RESID, a2, nb, s)) return 1;
    }
    GemmF32Args g5 = {};
    g5.A = w.y; g5.lda = HD; g5.sA = sy; g5.W = h->co_w; g5.ldw = HD; g5.C = w.feat; g5.ldc = OD; g5.sC = sfeat; g5.M = Tc; g5.Ms = Ts; g5.N = OD; g5.K = HD;
    if (launch_gemm_f32(EP_NONE, g5, nb, s)) return 1;                                     // encoder.conv_out 1x1
    if (any_feat) {
        hipLaunchKernelGGL(feat_out_batch_kernel, dim3(Tc, nb), dim3(256), 0, s, U, w.feat, sfeat, OD);
        CTTS_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(gfsq_batch_kernel, dim3(Tc, c.vq_groups, nb), dim3(64), 0, s, U, w.feat, sfeat, h->pin_w, h->pin_b, OD / c.vq_groups, OD, c.vq_residuals, c.pre_bound);
    CTTS_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int ctts_dvae_encode_batch(ctts_enc* h, const float* const* wav_ptrs, const int32_t* n_samples, int B, int32_t* const* ids_ptrs,
                                      float* const* mel_ptrs, float* const* feat_ptrs, void* stream) {
    if (!h || !h->finalized || !wav_ptrs || !n_samples || !ids_ptrs) { ctts_set_error("dvae_encode_batch: bad argument"); return 1; }
    if (B < 1 || B > CTTS_ENC_MAX_BATCH) { ctts_set_error("dvae_encode_batch: B=%d outside [1, %d]", B, CTTS_ENC_MAX_BATCH); return 1; }
    CTTS_RANGE("ctts_dvae_encode_batch");
    const ctts_enc_cfg& c = h->cfg;
    // every check before the first launch: a refused call leaves nothing half-written
    for (int u = 0; u < B; ++u) {
        if (n_samples[u] <= c.n_fft / 2 || n_samples[u] > c.max_samples) {
            ctts_set_error("dvae_encode_batch: utterance %d has %d samples, outside (%d, %d]", u, n_samples[u], c.n_fft / 2, c.max_samples);
            return 1;
        }
        if (!wav_ptrs[u] || !ids_ptrs[u]) { ctts_set_error("dvae_encode_batch: utterance %d has a null %s pointer", u, wav_ptrs[u] ? "ids" : "wav"); return 1; }
    }
    hipStream_t s = (hipStream_t)stream;
    // tables, staged in a pinned ring slot (a slot is reused only after its copy has run)
    const int slot = h->pin_next++ % 4;
    if (h->pin_used[slot]) CTTS_HIP_CHECK(hipEventSynchronize(h->pin_ev[slot]));
    char* p = h->pin + (size_t)slot * ENC_TAB_BYTES;
    EncUtt* U = (EncUtt*)p;
    int *Fs = (int*)(p + (size_t)CTTS_ENC_MAX_BATCH * sizeof(EncUtt)), *Ts = Fs + CTTS_ENC_MAX_BATCH;
    int Fall = 0;
    for (int u = 0; u < B; ++u) {
        const int F = 1 + n_samples[u] / c.hop, T = (F - 2) / 2 + 1;
        U[u] = {wav_ptrs[u], (int*)ids_ptrs[u], mel_ptrs ? mel_ptrs[u] : nullptr, feat_ptrs ? feat_ptrs[u] : nullptr, n_samples[u], F, T, 0};
        Fs[u] = F; Ts[u] = T;
        Fall = F > Fall ? F : Fall;
    }
    // the single-clip workspace is the minimum budget; a batch that does not fit it in one chunk gets the larger set, once
    if (!h->ws_big && !enc_fits(h->ws, enc_region(c, Fall), (size_t)B)) {
        const EncRegion r = enc_region(c, h->Fmax);
        ctts_enc::Ws w = {};
        w.n_xp = ENC_BATCH_WS * r.n_xp; w.rowsF = ENC_BATCH_WS * r.rowsF; w.rowsD1 = ENC_BATCH_WS * r.rowsD1; w.rowsT = ENC_BATCH_WS * r.rowsT;
        if (ealloc(h, &w.xp, w.n_xp) || ealloc(h, &w.spec, w.rowsF * h->spec_ld) || ealloc(h, &w.mag, w.rowsF * h->mag_ld) ||
            ealloc(h, &w.melcl, w.rowsF * h->mel_ld) || ealloc(h, &w.d1, w.rowsD1 * c.dim) || ealloc(h, &w.x2, w.rowsT * c.dim) ||
            ealloc(h, &w.b128, w.rowsT * c.enc_bn) || ealloc(h, &w.y, w.rowsT * c.enc_hidden) || ealloc(h, &w.ln, w.rowsT * c.enc_hidden) ||
            ealloc(h, &w.mid, w.rowsT * c.enc_hidden * 4) || ealloc(h, &w.feat, w.rowsT * c.enc_odim))
            return 1;
        h->ws = w;
        h->ws_big = true;
    }
    CTTS_HIP_CHECK(hipMemcpyAsync(h->d_tab, p, ENC_TAB_BYTES, hipMemcpyHostToDevice, s));
    CTTS_HIP_CHECK(hipEventRecord(h->pin_ev[slot], s));
    h->pin_used[slot] = true;
    // greedy chunks in call order: an utterance joins the open chunk while the chunk, strided by its longest clip, still fits
    int u0 = 0, Fc = 0, Tc = 0, nmax = 0;
    bool any_mel = false, any_feat = false;
    for (int u = 0; u <= B; ++u) {
        if (u < B) {
            const int Fn = U[u].F > Fc ? U[u].F : Fc;
            if (u == u0 || enc_fits(h->ws, enc_region(c, Fn), (size_t)(u - u0 + 1))) {
                Fc = Fn; Tc = U[u].T > Tc ? U[u].T : Tc; nmax = U[u].n > nmax ? U[u].n : nmax;
                any_mel |= U[u].mel != nullptr; any_feat |= U[u].feat != nullptr;
                continue;
            }
        }
        if (encode_chunk(h, u0, u - u0, Fc, Tc, nmax, any_mel, any_feat, s)) return 1;
        if (u < B) { u0 = u; Fc = U[u].F; Tc = U[u].T; nmax = U[u].n; any_mel = U[u].mel != nullptr; any_feat = U[u].feat != nullptr; }
    }
    return 0;
}
