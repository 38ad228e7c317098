/*
 * ctts_hip.h -- C ABI of libctts_hip.so: the MI355X (gfx950) backend for the ChatTTS hot path.
 *
 * This is the drop-in boundary.  The reference selects a backend per model
 * through the YAML field `infer_type` (chattts_plus/pipelines/chattts_plus_pipeline.py:113-129);
 * its accelerated backend (chattts_plus/trt_models/) drives an opaque engine through
 *   create_kv_cache / predict / get_cur_kv_caches   (trt_models/llama_trt_model.py:25-35,77-81)
 *   TensorRTPredictor.predict(feed_dict, stream)     (trt_models/predictor.py:141-169)
 * with torch owning every user-visible buffer and the engine seeing raw data_ptr()s and a stream.
 * The functions below are what an `infer_type: "hip"` binding needs for the same path; each entry
 * cites the reference interface it replaces.  Python binding: chatttsplus_amd/_lib.py (ctypes);
 * see INTEGRATION.md for the reference-side stub.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; ctts_last_error() gives the text
 *     (reference: predictor.py:165-167 raises ValueError("ERROR: inference failed.")).
 *   - no C++ exceptions, no abort(), no torch types cross the ABI: plain pointers and sizes.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *   - device pointers are borrowed; the caller keeps them alive (predictor.py:91-115,162).
 *   - a handle is bound to the device that was current at create() and is not thread-safe.
 */
#ifndef CTTS_HIP_H
#define CTTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTTS_DTYPE_F32 0 /* parity mode: fp32 weights / KV / MFMA (v_mfma_f32_16x16x4_f32) */
#define CTTS_DTYPE_F16 1 /* performance mode: fp16 weights / KV, fp32 accumulate (reference GPU dtype, pipeline:37-41) */

#define CTTS_MAX_BATCH 128  /* sequences decoded together (reference caps at 4: pipeline:391-397) */
#define CTTS_NUM_VQ 4

const char* ctts_last_error(void);
int ctts_version(void);

/* ------------------------------------------------------------------------------------------ */
/* GPT: Llama-style code-token decoder + sampler (models/gpt.py, models/llama.py, processors.py) */
/* ------------------------------------------------------------------------------------------ */

typedef struct ctts_gpt ctts_gpt;

typedef struct {
    int32_t hidden;        /* 768   gpt_config.hidden_size        (configs/infer/chattts_plus.yaml:73) */
    int32_t inter;         /* 3072  gpt_config.intermediate_size  (:74) */
    int32_t heads;         /* 12    num_attention_heads           (:75)  head_dim must be 64 */
    int32_t layers;        /* 20    num_hidden_layers             (:76) */
    int32_t vocab_code;    /* 626   num_audio_tokens              (:81) */
    int32_t num_vq;        /* 4                                   (:82) */
    int32_t max_batch;     /* <= CTTS_MAX_BATCH sequences decoded together */
    int32_t max_seq;       /* KV capacity per sequence: prompt + max_new_token */
    int32_t dtype;         /* CTTS_DTYPE_* */
} ctts_gpt_cfg;

/* replaces models.GPT.__init__ / trt_models.GPT.__init__ (gpt.py:25-82) */
int ctts_gpt_create(const ctts_gpt_cfg* cfg, ctts_gpt** out);
void ctts_gpt_destroy(ctts_gpt* h);

/* Named engine options (the YAML's `kwargs.options` of the hip GPT; no counterpart in the reference -- the TensorRT path fixes such choices when
 * the engine is built, trt_models/llama_trt_model.py:25-81).  Explicit calls only: the product library reads no behaviour from the environment.
 *   "prefill_split_rows"  fp32 engines: prompt passes of >= this many rows use the 3-term fp16 split GEMMs (default 65: every pass of more than 64 rows; 384 until round 6; 0 = never; before finalize)
 *   "split_decode_rows"   fp32 engines: decode batches of >= this many rows (packed-residual path, >= 9 rows, no per-utterance adapters) run their projections on the fp16 matrix
 *                         pipes with head / tail fp16 operands -- 3 MFMAs per product at fp32-level accuracy, the prompt pass's arithmetic -- instead of exact-f32 MFMA
 *                         (default 9; 0 = never.  Set to 0 BEFORE finalize and the engine builds no head / tail weight images unless the prompt pass needs them)
 *   "split_nbg2_rows"     ... and from this many rows on (default 17) they take 32-row blocks instead of 16-row chunks
 *   "weight_prefetch_kb"  launch chain from 9 rows on (fp16 engines: 17): the o_proj launch carries extra workgroups that pull the gate|up launch's weights into L2, one per this
 *                         many KiB (default 96; 0 = none).  The other launches were tried as carriers and lose (profiles/r06_ab_weight_prefetch.jsonl)
 *   "valu_rows"           fp32 engines: decode batches of <= this many rows run their projections on the VALU instead of exact-f32 MFMA (default 2; 0..4)
 *   "persistent_rows"     decode batches of <= this many rows (<= 8; default 8 on fp32 engines, 5 on fp16 engines; up to 5 rows one (row, head) per attention workgroup, 6..8 rows
 *                         two, with contexts up to "persistent_pair_keys" = 704 / 576 / 448 keys at 6 / 7 / 8 rows) run the whole decoder stack of a step as ONE persistent
 *                         launch of 256 resident workgroups (persist_layer.hip; up to 1400 keys per key share -- longer contexts go back to the launch chain; the final
 *                         norm + code heads run inside the launch at <= 2 rows; the two-item workgroups of 6..8 rows keep 192 keys of an item in registers and 128 more in LDS).
 *                         0 = off.  The first
 *                         process that loads an engine (either dtype) on a device holds the mode (advisory lock /tmp/ctts_persist_<pci>.lock); others stay on launches.
 *                         A persistent launch needs all 256 workgroups resident: run ONE decode at a time per device (two engines of one process decoding
 *                         concurrently on different streams would have to share the CUs; every wait is bounded and ctts_gpt_progress reports a give-up)
 *   "persistent_share_keys"  1..5 rows: one key share per (row, head) serves up to this + 128 cached keys (384 in registers, the rest in LDS), longer contexts open more shares (default 384)
 *   "persistent_lora"     1 (default): rows that carry a per-utterance adapter stay on the persistent launch -- its otherwise idle compute waves evaluate A h, the edge lanes add
 *                         B (A h) to their q / k / v / o_proj rows (paced schedule; 0 = such batches take the launch chain's worker workgroups, "lora_fold").
 *                         The launch carries the q/k/v/o terms only: while a live row's adapter names gate_proj / up_proj / down_proj the step takes the launch
 *                         chain at every row count, whatever this option says.  Teaching the persistent launch the MLP terms is out of scope so far; its price,
 *                         fp32, 1 row, ~300 keys: 0.897 ms/step with an all-seven-target adapter (launch chain) against 0.304 with a q/k/v/o adapter (persistent
 *                         launch; this library -- the parent commit's measured 0.316 in the same call; profiles/mlp_lora_probe.jsonl)
 *   "persistent_delay_lora"  poll delay of that hand-off (-1 = 14 + 2 rows, the default)
 *   "persistent_layers_per_launch"  0 = the whole stack in one launch (default), n = n layers per launch
 *   "persistent_schedule" weight request schedule of the persistent launch (1 / 2 / 3, default 3 = paced requests)    "persistent_pace"  its pacing interval (-1 = by row count, the default)
 *   "persistent_delay", "persistent_delay_act", "persistent_delay_x", "persistent_delay_att", "persistent_nap", "persistent_nap_qkv"  when and how often the edge waves poll
 *   "persistent_poll"     0 / 1: sentinel granules before the full sweeps (default 0)
 *   "persistent_timestamps" diagnostics: the persistent launches record per-workgroup phase marks
 *   "prefill_pp_blocks"   fp32 engines, prompt pass: a split GEMM may run on 256-row blocks with two counter-phased wave groups (prefill_split.hip) when it has at
 *                         least this many such blocks and the round count on 256 CUs favours it (default 1; 0 = 128 x 128 blocks only; -4 / -3 = always, with
 *                         that many n tiles per wave: tests).  All shapes give bit-identical results
 *   "prefill_splitk_rows" fp32 engines, prompt pass: passes of <= this many rows slice the down projection's K = 3072 four ways and add the slices in order (default
 *                         2048; 0 = never): 6 blocks per 128 rows otherwise walk 96 k-tiles each -- an 8 x 56-token pass 3.4 -> 2.4 ms.  Another summation order
 *                         than the unsliced kernel's (hidden rows move by ~1e-6; token ids unchanged on every golden)
 *   "prefill_small_blocks" / "prefill_ring4_blocks"   fp32 engines, short prompt passes: a split GEMM of at most this many 128 x 128 blocks (K slices counted) runs on 64 x 64
 *                         blocks (default 192: four times the blocks for grids that leave most CUs idle) / on a 4-stage LDS ring, one block per CU (default 256); 0 = never.
 *                         Bit-identical to the other block shapes
 *   "attn_wide_blocks"    unsplit decode attention takes 8-wave blocks while rows x heads < this (default 512 on fp32 engines, 4096 on fp16 engines; 0 = 256, the limit until round 6)
 *   "decode_splits"       key splits of the decode attention (0 = policy)       "split_rows"  split-K down projection as launch slices up to this batch size (default 8)
 *   "down_splitk_rows"    packed-residual decode batches of >= this many rows slice the down projection's K inside the launch, last arriver combines (default 9; 0 = never)
 *   "nbg2_rows"           decode batches of >= this many rows use 32-row blocks instead of 16-row chunks (default 81 fp32 / 57 fp16)
 *   "graph_steps"         decode steps captured per hipGraph (default 4)
 *   "graph_steps_persistent"  ... per hipGraph of the persistent paths, whose step is 2 launches (default 16; shorter remainders use "graph_steps")
 *   "lora_mlp_live"       read only (get_option): 1 while a live row's adapter names gate_proj / up_proj / down_proj
 *   "lora_fold"           per-utterance adapters at decode: 1 (default) = the rows' low-rank terms come from worker workgroups inside the QKV / o_proj launches
 *                         (lora_worker.h), 0 = two more launches per layer (lora.hip; the prompt pass always uses those).  The q/k/v/o terms only: gate / up / down
 *                         terms always come from two launches of their own per layer, beside either form (measured with all seven targets on every row, fp32,
 *                         ms/step 1 / 0: 1 row 0.90 / 1.06, 8 rows 1.04 / 1.24, 32 rows 1.19 / 1.39 -- the workers stay)
 *   "persistent_fault"    test hook: one workgroup withholds a hand-off in layer value - 1 (the bounded waits must end the step with an error)
 *   "batch_invariant"     fp32 (parity) engines, default 0 (fp16 engines: setting it is an error).  1 = the batch-invariance contract below.  Before or after
 *                         finalize (after: the engine must hold the head / tail weight images).
 *       CONTRACT (device noise, ctts_gen_io.noise == NULL; one engine = weights + max_seq): an utterance's hidden rows, token ids, end_idx -- and the mel computed
 *       from them -- are identical BIT FOR BIT whatever the schedule.  They are a function of its own inputs only (prompt ids, speaker, sampling parameters,
 *       token limit, utterance id, attempt), not of: the batch size, max_batch or its row; the other utterances of the batch, their prompt lengths (the left
 *       padding); finished-row compaction (ctts_gpt_compact); being started by ctts_gpt_begin or seated by ctts_gpt_admit, and at which step; the service
 *       order, slice size or number of ranks of the host.  (The repetition-penalty row quirk, SURVEY F8, needs >= 157 rows: beyond CTTS_MAX_BATCH.)
 *       How: every choice that depended on the row count, the pass height or the padding is pinned -- decode projections on the 3-term fp16 head / tail split
 *       MFMAs in 16-row chunks at every row count (1..8 rows too, one padded chunk), the down projection's K always sliced 4 ways with the fixed-order
 *       last-arriver combine, layer 0's q|k|v and the heads in one form, decode attention unsplit on 8-wave blocks (key loop anchored at the row's first
 *       real key), no persistent launch, no VALU rows; every prompt pass on the split GEMMs of prefill_split.hip (the 1-row pass too), K never sliced, the
 *       prompt attention's 64-key chunks anchored at the first real key; ctts_gpt_prefill passes T - 1 prompt tokens and the last one runs through the
 *       layer pass of the first decode step (ctts_gpt_sample), exactly as after ctts_gpt_admit (ctts_gpt_restart replays that pass).
 *       While the option is on, the tuning options it pins are IGNORED (their stored values return when it is switched off) and ctts_gpt_get_option reads the
 *       effective values: persistent_rows 0, valu_rows 0, split_decode_rows 1, split_rows 0, down_splitk_rows 1, nbg2_rows / split_nbg2_rows 0 (never),
 *       decode_splits 1, attn_wide_blocks INT_MAX, prefill_split_rows 1, prefill_splitk_rows 0.  Block-shape options (prefill_pp_blocks, prefill_small_blocks,
 *       prefill_ring4_blocks, weight_prefetch_kb) stay live: they do not change the arithmetic.
 *       An utterance's sampling knobs (ctts_gpt_set_row_sampling / ctts_gpt_admit_sampling) count as its own inputs: they are covered like its token limit.
 *       Sharing a prompt pass (ctts_gpt_share_prompts) is one more thing an utterance's outputs do not depend on: a prompt row's K / V is a function of the
 *       utterance's own inputs, so the lane a follower receives is bit for bit what its own prompt pass would have written.
 *       OUTSIDE the contract: caller-supplied noise (indexed by the batch's draw counter); per-utterance adapters (ctts_gpt_set_row_adapters /
 *       ctts_gpt_admit_adapters: begin / admit with a live adapter row return an error naming the option; a merged adapter, ctts_gpt_merge_lora, is just
 *       weights and is covered); ensure_non_empty restarts of a whole generate() batch (ctts_gpt_restart: the reference regenerates the slice, so an
 *       utterance's attempt number depends on its slice -- reference semantics).  The refine-text pass (infer_text) runs the same pinned stack and is covered.
 *       A checkpoint with a weight beyond the fp16 range (x 64) cannot take the option (begin returns an error).
 *       Scoring (ctts_gpt_score) is covered too: a sequence's logprob and argmax are identical bit for bit whatever the batch size, its row, the other
 *       sequences' padding and the pass boundaries (the prompt pass pinned as above, the code heads on 16-row chunks at every row count).
 * Unknown names are an error. */
int ctts_gpt_set_option(ctts_gpt* h, const char* name, int value);
int ctts_gpt_get_option(ctts_gpt* h, const char* name, int* value);      /* every option that can be set can be read; the EFFECTIVE value ("persistent_rows" reads 0 where the mode is unavailable) */

/* One more option, the dtype-independent name of the contract above: "schedule_invariant" (flag, default 0, read / write, before or after finalize; part of the
 * decode-graph key like every option).
 *   fp32 engines: a synonym of "batch_invariant" -- the same field, the same hook, the same refusals; either name reads what the other set.
 *   fp16 engines: the ONLY accepted setter (setting "batch_invariant" there stays an error, whose message names this option).  While it is on,
 *       get_option("batch_invariant") reads 1 too -- reading was never refused -- so hosts that ask "does this engine keep the contract?" under the older
 *       name (share_prompt=None of infer(num_candidates=N), the sessions, generate_many) need no change.
 * With the option at 0 every engine launches exactly what it launched without it.
 * The CONTRACT on fp16 engines is the one stated above, word for word: under device noise an utterance's hidden rows, token ids, end_idx and log-probs are bit
 * for bit a function of its own inputs only -- not of the batch size, max_batch, its row or KV lane; the other utterances and their padding; compaction, begin
 * versus admit, grow, or the cancel of other rows; the service order, slice size or rank count; the pass boundaries of the prompt pass; shared prompt passes.
 * Scoring (ctts_gpt_score: logprob, argmax), the refine-text pass and text rows beside code rows are covered as on fp32 engines.  Values are fp16-mode values:
 * the option changes which fp16 kernels run, not their precision (mel / waveform against the CPU oracle stay within the fp16 mode's 2e-3).
 * How, on fp16 engines -- no head / tail weight images are involved, and no message that demands them fires:
 *   decode  the launch chain at every row count on the packed fp16 residual stream (EPI_RESID_XH -> PRO_XH) in 16-row chunks (1..8 rows: one padded chunk; never
 *       32-row blocks), the down projection's K always sliced four ways inside the launch with the fixed-order last-arriver combine (EPI_RESID_XH_SK), never
 *       split-K launch slices, layer 0's q|k|v (PRO_NORM) and the code heads (PRO_XH) / text head (PRO_NORM_P) on 16-row chunks in one prologue form each,
 *       decode attention unsplit (S = 1) on 8-wave blocks, no persistent launch (its weight images are never built).  The weight-prefetch workgroups stay
 *       live ("weight_prefetch_kb", from 17 rows): they do no arithmetic.  No pin beyond this list turned out to be needed.
 *   prompt  ONE projection arithmetic at every pass height, the 1-row pass included: norm_pack, then the LDS-staged GEMM of prefill_gemm.hip -- every output is
 *       accumulated by one wave in k order, rows past the end are clamped, K is never sliced -- pinned to its 128 x 128 blocks (the taller shapes share the
 *       k order; the choice by pass height is switched off all the same).  The MFMA flash attention at every pass height too, its 64-key chunks anchored at
 *       the sequence's first real key; a chunk outside a query's own [first real key, slot] leaves that query's state bit-unchanged, so the queries that happen
 *       to share its 64-query block do not matter.  ctts_gpt_prefill passes T - 1 prompt tokens, the last one runs through the first decode step's layer pass
 *       (ctts_gpt_sample), exactly as after ctts_gpt_admit; ctts_gpt_restart replays that pass; ctts_gpt_score runs its heads on 16-row chunks.
 *   fp16 saturating stores and ctts_gpt_saturations behave as without the option.
 * ctts_gpt_get_option while the option is on, fp16 engines: persistent_rows 0, split_rows 0, down_splitk_rows 1, nbg2_rows 0 (never), decode_splits 1,
 * attn_wide_blocks INT_MAX, prefill_splitk_rows 0; the fp32-only mechanisms read what "never used" reads: split_decode_rows 0, prefill_split_rows 0 (fp32 engines:
 * 1 and 1), split_nbg2_rows 0, valu_rows 0.  Stored values return when the option is switched off.
 * OUTSIDE the contract, and refused with a message naming the option: per-utterance adapters (ctts_gpt_set_row_adapters / ctts_gpt_admit_adapters, begin / admit
 * with a live adapter row), as on fp32 engines; caller-supplied noise -- fp16 engines refuse it at ctts_gpt_begin (fp32 engines keep accepting it: their
 * reference goldens replay torch's draws under the option; it is outside the contract there as well). */

/* Diagnostics (tools/persist_probe.py): copies a named internal buffer to HOST memory -- "x_dec", "q_buf", "logits", "meta_dec" ({KV lane, pos, slot, kv_start} per decode row), "pl_g" (the persistent
 * layer's granule buffers), "pl_ts" (its per-workgroup phase marks, option "persistent_timestamps"), "pl_state" ({epoch, error}), "xh" / "ssq" (the packed residual copy and its per-tile sums of squares).  Synchronises.
 * "decode_plan" is computed on the host (no device work, no synchronisation, no effect on any launch): the launch plan of a decode step of the current batch on the path
 * of the last step the last ctts_gpt_decode call planned, as 23 int32 in this order -- B, path.splits, path.persist, then the layer plan S, nbg, chunks, dts, pf_kb, valu,
 * wide_blocks, splitd, prepack, xhm, spd, down_sk, fuse_heads, lora, then the residual stream's form for the heads parts, xh, logits, split, nbg, valu.  An error before the
 * first decode call of a batch.
 * "prompt_plan" likewise (host only): the launch plans of the prompt passes of the last ctts_gpt_prefill / ctts_gpt_score call, as 34 int32 -- passes, rows of a full pass,
 * rows of the last pass, tokens per sequence of the prompt rows (T; T - 1 under "batch_invariant" / "schedule_invariant"), then for each of the two pass heights (full, last)
 * nbg, prepack, pfg, pfs, anchor, lora, the attention kind (0 row kernel, 1 MFMA flash, 2 MFMA flash anchored, 3 split kernel) and for each of qkv, o, gate|up, down a GEMM
 * kind (0 tile kernel with the norm in the block, 1 tile kernel on the packed operand, 2 / 3 / 4 prefill_gemm shape 0 / 1 / 2, 5 split 64 x 64, 6 split ring4, 7 split ring2,
 * 8 split pp3, 9 split pp4) and `sliced`.  "meta_pre": the RowMeta {KV lane, pos, slot, kv_start} of every prompt row of that call; "x_pre": the fp32 residual rows its
 * last pass left, rows x H (both synchronise).  All three are an error while no prompt pass has run since ctts_gpt_begin. */
int ctts_gpt_debug_read(ctts_gpt* h, const char* name, void* out, size_t max_bytes, size_t* bytes, void* stream);

/* replaces GPT.from_pretrained -> load_state_dict (gpt.py:84-85).  `name` is the reference
 * state-dict key; `data` is HOST fp32, row-major, `numel` elements.
 * Accepted keys: gpt.layers.N.{self_attn.{q,k,v,o}_proj,mlp.{gate,up,down}_proj,input_layernorm,
 * post_attention_layernorm}.weight, gpt.norm.weight, emb_code.N.weight,
 * emb_text.weight, head_code.N.parametrizations.weight.original{0,1}, head_text.parametrizations.weight.original{0,1}
 * (the last two + emb_text enable the refine-text pass, infer_text=1). */
int ctts_gpt_set_weight(ctts_gpt* h, const char* name, const float* data, size_t numel);

/* LoRA merge rule of peft merge_and_unload (pipeline:420-432): W += scale * B @ A for one target of one layer -- "q_proj", "k_proj", "v_proj", "o_proj"
 * (out x in = hidden x hidden), "gate_proj", "up_proj" (intermediate x hidden) or "down_proj" (hidden x intermediate; llama.py:214,737-739).  A [r][in], B [out][r], host
 * fp32, both sized by the TARGET's own (out, in): the caller checks the shapes (hip_models.GPT.add_lora does).  An unknown target or a layer whose matrix is not loaded is
 * an error naming it.  Call before finalize: a merged adapter is just weights, every engine mode serves it. */
int ctts_gpt_merge_lora(ctts_gpt* h, int layer, const char* target, const float* A, const float* B, int r, float scale);

/* Per-utterance LoRA (no counterpart in the reference, which merges ONE adapter for a whole batch, pipeline:420-432):
 * up to CTTS_MAX_ADAPTERS adapters stay resident beside the packed weights; every sequence of a batch selects one slot or none and
 * the projections evaluate  W x + scale * B (A x)  per row.  Call after ctts_gpt_finalize.
 *   set_adapter      one (layer, target) of adapter `slot`; targets and shapes as for ctts_gpt_merge_lora (A [r][in], B [out][r], host fp32), r <= 16.
 *                    The tables of gate_proj / up_proj / down_proj (737 KB per layer and slot in fp32, 118 MB for 20 layers x 8 slots) are allocated when the
 *                    first such target is loaded; the rows' gate / up terms (24 KB per prompt row of a pass: 402 MB on an engine sized for 16384-row passes)
 *                    when a live row first selects a slot that holds one.  While a LIVE row's slot holds one of them, every layer runs two more launches (lora.hip:
 *                    the gate / up term from the post-attention RMSNorm output, added before the activation in the SwiGLU epilogues; the down term from the
 *                    down projection's own packed operand, added with the residual) -- decode steps and prompt passes -- and decode steps take the launch chain
 *                    at every row count ("persistent_lora").  A batch whose live rows use q/k/v/o adapters only, or none, launches exactly what it would
 *                    with no MLP adapter resident.
 *   clear_adapter    zeroes a slot (all layers / targets)
 *   set_row_adapters slot (or -1) per sequence for the following ctts_gpt_begin calls; slots == NULL or B == 0 switches the path off */
#define CTTS_MAX_ADAPTERS 8
int ctts_gpt_set_adapter(ctts_gpt* h, int slot, int layer, const char* target, const float* A, const float* B, int r, float scale);
int ctts_gpt_clear_adapter(ctts_gpt* h, int slot);
int ctts_gpt_set_row_adapters(ctts_gpt* h, const int32_t* slots, int B);

/* folds weight-norm heads (W = g*v/||v||_row, gpt.py:57-77), packs QKV / gate|up, converts to the
 * engine dtype, uploads.  After this the host copies are released. */
int ctts_gpt_finalize(ctts_gpt* h);

/* bytes of KV cache the caller must provide: [layers][2][max_batch][heads][max_seq][64] of dtype.
 * replaces LlamaTRTModel.create_kv_cache (llama_trt_model.py:25-29). */
size_t ctts_gpt_kv_bytes(const ctts_gpt* h);
int ctts_gpt_bind_kv(ctts_gpt* h, void* kv_dev, size_t bytes);

/* RoPE table [max_seq][64] fp32 = (cos[32], sin[32]) of pos*inv_freq, computed by the caller with the
 * reference's fp32 arithmetic (llama.py:100,106-119) so that the values are bit-identical to the CPU path. */
int ctts_gpt_set_rope(ctts_gpt* h, const float* rope_host, int n_pos);

typedef struct {
    float temperature[CTTS_NUM_VQ];   /* per-codebook temperature (gpt.py:346-351) */
    float top_p_threshold;            /* (float)(1 - top_P) as torch compares it (TopPLogitsWarper); <0 disables top-p */
    int32_t top_k;                    /* max(top_K, min_tokens_to_keep) (TopKLogitsWarper); <=0 disables */
    int32_t min_tokens_to_keep;       /* 3 (processors.py:45,47) */
    int32_t use_penalty;              /* repetition_penalty != 1 (processors.py:50) */
    float penalty_table[17];          /* penalty**n, n=0..16, as torch.pow(float, int64) gives (processors.py:28) */
    int32_t past_window;              /* 16 (processors.py:53) */
    int32_t max_input_ids;            /* row-count quirk threshold (processors.py:23-27) */
    int32_t eos_token;                /* num_embeddings-1 = 625 (pipeline:209) */
    int32_t min_new_token;            /* (gpt.py:477-478) */
    int32_t max_new_token;
    int32_t infer_text;               /* 1: refine-text pass (gpt.py infer_text=True: 21178-way head_text, temperature[0] only,
                                         next input = emb_text[id], use_penalty must be 0); noise is then [n_draws][B][vocab_text] */
} ctts_sampler_cfg;

/* Per-utterance sampling knobs (no counterpart in the reference, whose InferCodeParams apply to a whole call): one entry per sequence, the same
 * fields and conversions as ctts_sampler_cfg.  Per utterance: temperature, top-p, top-k, min_tokens_to_keep, the repetition penalty (its table and
 * window) and min_new_token.  Per call (ctts_sampler_cfg): eos_token, max_input_ids (the F8 row quirk: a property of the batch row), max_new_token,
 * infer_text.  Code mode only: the refine-text pass keeps the call's values (begin refuses per-row knobs with infer_text).  Invalid entries
 * (temperature <= 0 or not finite, top_k < 0, min_tokens_to_keep < 1, past_window outside 1..16, min_new_token > max_new_token) are an error.
 * Cost: the sampler branches per sequence (one block) between its <= 64-candidate path and the serial one, so mixed knobs add no divergence inside
 * a wave -- but a batch that holds one row with top_k 0 (disabled) or > 64 runs at the speed of that row's serial path.  112 bytes (7 x 16). */
typedef struct {
    float temperature[CTTS_NUM_VQ];   /* per codebook, > 0 */
    float top_p_threshold;            /* (float)(1 - top_P); < 0 disables top-p */
    int32_t top_k;                    /* max(top_K, min_tokens_to_keep); 0 disables top-k */
    int32_t min_tokens_to_keep;       /* >= 1 (3 as processors.py builds it) */
    int32_t use_penalty;              /* repetition_penalty != 1 */
    float penalty_table[17];          /* penalty**n, n = 0..16, as torch.pow(float, int64) gives */
    int32_t past_window;              /* 1..16 */
    int32_t min_new_token;            /* <= the call's max_new_token */
    int32_t reserved;                 /* 0 */
} ctts_row_sampling;

/* Outputs of one generate() call, all device memory provided by the caller:
 *   ids      int32 [B][max_new_token][4]     (gpt.py:368-376 inputs_ids_buf, generated part)
 *   hiddens  fp32  [B][max_new_token][hidden] (gpt.py:422-423, post final norm)
 *   finish   int32 [B], end_idx int32 [B]    (gpt.py:339-342,486-487,530-531)
 * noise: fp32 [n_draws][B*4][vocab_code] Exp(1) draws consumed one per sample step (argmax(p/q) ==
 * torch.multinomial), or NULL for the on-device Philox generator seeded with `seed`.
 * utt_ids (device noise only): HOST array [B] of caller-chosen global utterance ids, or NULL for 0..B-1.  The Philox stream of a
 * sequence is keyed by (seed, its utterance id, codebook, its own step, its own regenerate attempt) -- not by its row in the batch and
 * not by the batch's draw counter -- so a request gives every utterance the same noise whatever slice, batch position or rank it is
 * served in (the reference's independence argument for slices: pipeline:391-397). */
typedef struct {
    int32_t* ids;
    float* hiddens;
    int32_t* finish;
    int32_t* end_idx;
    const float* noise;
    int32_t n_draws;
    uint64_t seed;
    const uint64_t* utt_ids;
    const int32_t* row_limits;      /* HOST array [B] or NULL: per-utterance token limit (<= max_new_token): the sequence counts as finished once it
                                       has produced that many tokens -- the per-row form of the loop bound gpt.py:389 */
} ctts_gen_io;

/* GPT.forward / get_emb (gpt.py:125-149) fused with Tokenizer.apply_spk_emb (tokenizer.py:150-178):
 * input_ids int32 [B][T][4] device, text_mask int32 [B][T] device (1 = text row -> emb_text, 0 = code row -> sum of the
 * 4 code embeddings); rows whose first id == spk_id receive spk fp32 [B][hidden] (already L2-normalised; NULL = none).
 * emb_out fp32 [B][T][hidden] device.  Ids must be < the table sizes (no bounds check on the device). */
int ctts_gpt_embed(ctts_gpt* h, const int32_t* input_ids_dev, const int32_t* text_mask_dev, int B, int T, const float* spk_dev, int spk_id,
                   float* emb_out_dev, void* stream);

/* Start a generate() call for B sequences with a T-token (left padded) prompt.
 * attention_mask int32 [B][T] device (1 = token, 0 = pad; tokenizer.py:96-115).
 * replaces the set-up part of GPT.generate (gpt.py:335-387). */
int ctts_gpt_begin(ctts_gpt* h, int B, int T, const int32_t* attention_mask_dev, const ctts_sampler_cfg* sc,
                   const ctts_gen_io* io, void* stream);

/* Prompt pass: emb fp32 [B][T][hidden] device (GPT.forward output after apply_spk_emb, gpt.py:125-149,
 * tokenizer.py:150-178).  Fills the KV cache and leaves the last position's residual row per sequence.
 * Asynchronous with respect to the host (enqueues on `stream`, never synchronises); prompts of more than 16384 rows (B * T) run in
 * several passes.  fp16 engines use the MFMA flash-attention kernel from 64 rows and the LDS-staged prompt GEMM from 1536 rows; fp32
 * (parity) engines run the same tiling on head / tail fp16 operand images from 384 rows (three fp16 MFMAs per product, fp32-accurate, fp32 KV
 * cache; prefill_split.hip); smaller prompts go through the decode kernels in 32-row chunks.
 * replaces the i == 0 iteration's LlamaModel.forward (gpt.py:410-418; llama.py:905-1019). */
int ctts_gpt_prefill(ctts_gpt* h, const float* emb_dev, void* stream);

/* Teacher-forced scoring of audio codes (the evaluation of train_lora.py:430-469: GPT.forward -> gpt.gpt.forward -> head_code[i], then cross-entropy
 * and argmax accuracy over the code tokens).  Inference only: there is no backward pass.
 *   attention_mask int32 [B][T] device, LEFT padded; emb fp32 [B][T][hidden] device (ctts_gpt_embed: text rows and code rows, the layout
 *   Tokenizer.encode gives a zero-shot prompt whose audio codes follow the text).  Sequence b has n_targets_host[b] = n_b targets (HOST array [B]);
 *   targets int32 [B][max_targets][4] device.  The final-normed hidden row at position T - n_b + j predicts target j (0 <= j < n_b); per codebook c:
 *     logprob[b][j][c] = log_softmax(head_code[c](hidden))[targets[b][j][c]]   on the RAW logits (no temperature, penalty, top-P / top-K)
 *     argmax[b][j][c]  = the first index of the largest logit (torch.argmax)
 *   both [B][max_targets][4] device.  Entries j >= n_b are written as 0 and -1; a target outside [0, vocab_code) gives NaN and -1 (no logit is read for it).
 * Positions are cumsum(mask) - 1 with pads at 1, exactly as ctts_gpt_begin computes them, so a sequence scores the same alone as left padded inside a
 * batch.  (train_lora.py:439 passes no position_ids, so its forward uses arange, llama.py:953-954: the two agree for unpadded rows only.)
 * Errors naming the limit: B > max_batch, T > max_seq, n_b < 1, n_b > T, n_b > max_targets, a handle that is not ready.
 * The call overwrites KV lanes 0..B-1 and the prompt-pass workspaces: it ENDS any generate state (sample, decode, admit, ... need a new
 * ctts_gpt_begin, as after create).  It honours the slots of ctts_gpt_set_row_adapters per sequence, as begin does.  fp32 and fp16 engines; the code
 * heads only.  The first call allocates a scratch of 2048 x (hidden + 4 * vocab_code + 1) words (27 MB at the real widths).  Asynchronous: never
 * synchronises.  Under "batch_invariant" see the CONTRACT above. */
int ctts_gpt_score(ctts_gpt* h, int B, int T, const int32_t* attention_mask_dev, const float* emb_dev, const int32_t* targets_dev,
                   const int32_t* n_targets_host, int max_targets, float* logprob_dev, int32_t* argmax_dev, void* stream);

/* Teacher-forced scoring under the refine-text head: ctts_gpt_score's layout and position rule -- the final-normed hidden row at T - n_b + j predicts target j --
 * with targets int32 [B][max_targets] and ONE column of results:
 *     logprob[b][j] = log_softmax(head_text(hidden))[targets[b][j]]   on the raw vocab_text_head-wide row;   argmax[b][j] = the first index of its largest logit
 * both [B][max_targets] device; unused entries and out-of-range targets (here: outside [0, vocab_text_head)) as in ctts_gpt_score.
 * The gathered rows go through the text-head launch of a decode step (final RMSNorm + weight-normed head_text, PRO_NORM / EPI_LOGITS) in chunks of at most
 * max_batch rows (option "score_text_chunk", read only) into a logits scratch, which one workgroup per row reduces (first index of the maximum, sum of expf in
 * fp32): log-probs agree with the lp_raw that ctts_gpt_set_text_logprob_out wrote for the same tokens to the decode-against-prompt-pass tolerance.  The first
 * call allocates the scratch, max_batch x (hidden + vocab_text_head + 1) words (11 MB at 128 rows); engines that never call it allocate nothing more.
 * Everything else -- adapter slots, the end of any generate state, engines, asynchrony, errors -- is ctts_gpt_score's: the two entry points share one routine
 * (gpt_engine.hip score_rows).  One more error: an engine without head_text.* / emb_text.weight.  A fused head with an online log-sum-exp that never
 * writes the logits is the faster shape for long targets and is not built here (it changes the summation order against the decode step). */
int ctts_gpt_score_text(ctts_gpt* h, int B, int T, const int32_t* attention_mask_dev, const float* emb_dev, const int32_t* targets_dev,
                        const int32_t* n_targets_host, int max_targets, float* logprob_dev, int32_t* argmax_dev, void* stream);

/* Sample phase for the current hidden rows: final RMSNorm + 4 folded heads + sampler chain +
 * EOS/finish bookkeeping + next-token embedding (gpt.py:422-494,527-532).  Used once after prefill
 * (step 0) and again after an ensure_non_empty restart (gpt.py:496-525). */
int ctts_gpt_sample(ctts_gpt* h, void* stream);

/* Reset step/finish state and re-gather the prompt's last hidden rows (ensure_non_empty regenerate);
 * the noise draw counter keeps running like torch's generator does in the reference. */
int ctts_gpt_restart(ctts_gpt* h, void* stream);

/* n_steps x { 20 decoder layers on the last sampled token ; sample phase } (gpt.py:389-546, i > 0).
 * use_graph != 0: replays captured hipGraphs of 4 steps each (cached per batch size / mode / KV binding / attention split
 * count; they contain no per-call state -- ctts_gpt_begin writes the output buffers, noise buffer, seed and sampling
 * parameters into a device block the kernels read -- so consecutive generate() calls reuse them); a remainder of < 4 steps
 * is launched kernel by kernel.  Steps after every sequence has finished exit early on the device.  Asynchronous w.r.t. the host. */
int ctts_gpt_decode(ctts_gpt* h, int n_steps, int use_graph, void* stream);

/* Host-visible progress: number of sample steps executed and whether every row has finished.
 * Synchronises the stream. */
int ctts_gpt_progress(ctts_gpt* h, int32_t* steps_done, int32_t* all_finished, void* stream);

/* fp16 engines store SwiGLU outputs and the packed residual copy as fp16: values beyond the fp16 range are SATURATED at +-65504 and
 * counted (the reference's .half() path would produce inf -> NaN silently on such a checkpoint, pipeline:37-41); `count` = saturated or NaN
 * stores since ctts_gpt_begin.  Synchronises the stream.  fp32 engines store fp32 everywhere EXCEPT in the prompt pass over >= 65 rows ("prefill_split_rows"), whose
 * split GEMMs keep silu(g) * u / 16 as fp16 head / tail images (prefill_split.hip): a value beyond +-65504 * 16 there is clamped and counted too
 * (the decode steps of an fp32 engine never count). */
int ctts_gpt_saturations(ctts_gpt* h, int32_t* count, void* stream);

/* Finished-row compaction (no counterpart in the reference, whose finished rows keep computing until the slowest sequence ends,
 * gpt.py:527-546): between two ctts_gpt_decode calls the caller may drop rows of the decode batch.
 *   rows_enqueue  copies {finish, end_idx} of the CURRENT rows (2 int32 each, row order) into pinned host memory, asynchronously
 *   compact       keep_rows = HOST array of n_keep current row indices, ascending; the engine re-packs its per-row state (residual
 *                 rows, positions, repetition-penalty windows, noise keys) so that they become rows 0..n_keep-1 and continues with a
 *                 batch of n_keep.  The KV cache and the output arrays are indexed by utterance and do not move.  Code mode only. */
int ctts_gpt_rows_enqueue(ctts_gpt* h, int32_t* host_pinned_2B, void* stream);
int ctts_gpt_compact(ctts_gpt* h, const int32_t* keep_rows, int n_keep, void* stream);

/* Continuous batching (no counterpart in the reference: its slices of 4 run one after the other, each to its slowest row,
 * pipeline:391-397): between two ctts_gpt_decode calls `n` NEW utterances take over decode rows whose utterance has finished (the
 * caller has seen their finish flag through rows_enqueue).
 *   rows        HOST [n] current row indices, distinct
 *   T, mask, emb   the new utterances' left-padded prompts: DEVICE mask [n,T] int32, emb [n,T,H] fp32 (ctts_gpt_embed); T + max_new_token
 *               must fit max_seq and n*(T-1) one prompt pass
 *   utt_ids, row_limits (may be null), out_index, attempts (may be null)   HOST [n]: noise key, token limit, place in the ids / hiddens /
 *               finish / end_idx arrays handed to ctts_gpt_begin (which must be large enough: they are indexed by out_index, not by
 *               row), regenerate attempt (ensure_non_empty: an utterance whose first token was EOS is admitted again with attempt + 1)
 * The prompt but its last token goes through a prompt pass into the rows' KV lanes; the last token becomes the rows' next decode input, so
 * the next decode step samples the utterance's first token.  Step counter, noise stream, limit and outputs are per row, so an utterance's
 * result does not depend on when or where it is admitted.  Device noise only.  Per-utterance adapters: name the new utterances' slots with
 * ctts_gpt_admit_adapters first.  Asynchronous. */
int ctts_gpt_admit(ctts_gpt* h, int n, const int32_t* rows, int T, const int32_t* mask, const float* emb, const uint64_t* utt_ids,
                   const int32_t* row_limits, const int32_t* out_index, const int32_t* attempts, void* stream);

/* Elastic batch and cancellation (no counterpart in the reference): what a serving session needs between two ctts_gpt_decode calls, next to compact and admit.
 * Both are asynchronous, never synchronise, and work in code mode and text mode alike.
 *   grow    appends `n` dead rows B .. B+n-1 to the decode batch (B + n <= max_batch).  A dead row is a finished row that holds no utterance: it counts as
 *           finished (ctts_gpt_progress, rows_enqueue report {1, 0}), writes nothing into the output arrays, carries the call's sampling knobs and no adapter,
 *           and is parked on slot 0 of a KV lane no row of the batch uses (the lowest free lanes of [0, max_batch): after a compaction these are not B ..).
 *           Seat utterances in the new rows with ctts_gpt_admit (+ admit_adapters / admit_sampling).  The next ctts_gpt_decode plans its launches, picks its
 *           graphs and its persistent-launch limit by the new row count, exactly as after ctts_gpt_compact; "batch_invariant" engines accept the call (the
 *           option pins every choice that depends on the row count).  Device noise only, as ctts_gpt_admit.  No ctts_gpt_restart afterwards.
 *   cancel  rows = HOST [n] current row indices, distinct.  Every named row that is still live becomes a finished row where it stands: finish[out] stays 0
 *           (EOS not seen), end_idx[out] keeps the number of tokens written, nothing more is written for it.  Rows that had already finished are left alone
 *           (decided on the device: the host cannot know).  The row count does not change, so the other rows' launches -- and results -- are those of the
 *           same schedule without the call.  When the last live row is cancelled the batch reports all-finished.
 * Both act on the generate state of the last ctts_gpt_begin, which outlives the call that began it: the output arrays handed to that begin (ids, hiddens, log-probs,
 * finish, end_idx) must still be alive when rows are grown and admitted, as for ctts_gpt_admit -- the engine keeps the pointers, not the memory.
 * Not offered inside one generate state: caller-supplied noise with grow; a session on top of these (GPT.open_session) additionally refuses shared prompt
 * passes / num_candidates, session-wide streaming windows (stream= at open_session: streaming is asked per utterance at submit, and vocoded through
 * ctts_synth_windows from the token counts ctts_gpt_rows_enqueue reports) and infer_sharded.  The refine-text pass runs INSIDE such a session as text rows beside the code rows
 * (ctts_gpt_enable_text_rows below; GPT.open_session(text_rows=...), submit(mode="text")). */
int ctts_gpt_grow(ctts_gpt* h, int n, void* stream);
int ctts_gpt_cancel(ctts_gpt* h, int n, const int32_t* rows_host, void* stream);

/* Adapter slots (ctts_gpt_set_adapter; -1 = none) of the utterances the NEXT ctts_gpt_admit call seats in `rows`; rows not named keep theirs.  When no
 * live row carries an adapter any more the engine drops back to the plain launches. */
int ctts_gpt_admit_adapters(ctts_gpt* h, int n, const int32_t* rows, const int32_t* slots, void* stream);

/* Per-utterance sampling knobs (ctts_row_sampling; no counterpart in the reference).
 *   set_row_sampling  HOST per_seq [B]: knobs of sequences 0..B-1 for the following ctts_gpt_begin calls (sequences beyond B, and every call after
 *                     per_seq == NULL / B == 0, take the call's ctts_sampler_cfg values).  The request persists until it is cleared; begin checks it.
 *   admit_sampling    HOST rows [n], p [n]: knobs of the utterances the NEXT ctts_gpt_admit call seats in `rows` (call it before the admit).  An admitted
 *                     row that is not named gets the call's values -- never the knobs of the finished utterance whose row it takes.
 * The knobs follow an utterance through ctts_gpt_compact and ctts_gpt_restart.  The sampler reads them per decode row from a table at a fixed
 * engine address, so captured decode graphs stay valid. */
int ctts_gpt_set_row_sampling(ctts_gpt* h, const ctts_row_sampling* per_seq, int B);
int ctts_gpt_admit_sampling(ctts_gpt* h, int n, const int32_t* rows, const ctts_row_sampling* p, void* stream);

/* Text rows beside code rows in one decode batch (no counterpart in the reference, which runs the refine-text pass as a call of its own, pipeline:237-277): the
 * mode is a property of the decode ROW (0 = code: four codebook rows, the code heads, the code sampler; 1 = text: one row under head_text, the refine-text
 * sampler, next input = emb_text[id]).  The 20-layer stack, the row record (own step, output slot, limit, utterance id, attempt), compact, grow, admit and cancel
 * are the same for both; only the sample phase differs.  The call itself is a CODE-mode call (its ctts_sampler_cfg has infer_text = 0), device noise.
 *   enable_text_rows  gives the generate state its text block: text_sc = the refine pass's parameters (infer_text = 1: temperature[0], top-P, top-K,
 *                     eos_token = [Ebreak], min_new_token, max_new_token = the text rows' limit) and text_ids_dev int32 [n_out][text max_new_token][4], the text
 *                     rows' ids (laid out as an infer_text call writes them: the id repeated over the 4 columns), n_out = the extent of the call's ids array.
 *                     Text utterances take their output slot from the SAME index space as code utterances -- a slot is held by one utterance of either kind --
 *                     and write finish / end_idx of the call at it.  The text rows' max_new_token must not exceed the code call's: a text row's own step
 *                     indexes the call's per-slot arrays (the heads write its hidden row at [slot][step] when hiddens are asked for; nobody reads it).
 *                     The first call allocates the text logits [max_batch][vocab_text] and the block; engines that never call it allocate what they did.
 *   set_row_modes     HOST modes [B]: modes of sequences 0..B-1 for the following ctts_gpt_begin calls (a persisting request, like set_row_sampling); NULL / 0
 *                     clears.  ORDER when begin itself seats a text row: set_row_modes, ctts_gpt_begin, ctts_gpt_enable_text_rows, (set_logprob_out,)
 *                     ctts_gpt_prefill, ctts_gpt_sample -- enable_text_rows needs the state begin creates and clamps the begun text rows' limits to the
 *                     text max_new_token; sample / decode refuse a batch that holds a text row without it.
 *   admit_modes       one-shot, like admit_sampling: modes of the utterances the NEXT ctts_gpt_admit seats in `rows`; rows not named become code rows (never the
 *                     mode of the finished utterance whose row they take).  A mode-1 entry needs enable_text_rows first.
 * A step is MIXED while a row of the batch has mode 1 (option "text_rows_live", read only: the number of such rows; a finished text row counts until it is
 * compacted away or its row is handed to a code utterance).  A mixed step runs two more launches: after the code heads, which run over all rows as in any step
 * (a text row's code logits are not read), the text head over all rows into the text logits; then the code sampler -- the blocks of text rows return after their
 * first loads -- and the text sampler on the text block -- the blocks of code rows return.  The persistent launch drops its fused heads in mixed steps (they leave
 * the stack's output in the launch's granules, not in the residual rows the text head reads), so at <= 2 rows the code heads are a third extra launch.  Every row takes
 * its arrival ticket once per step, in the kernel of its mode; the last arriver advances the step.  Unmixed steps launch exactly what they did.  Device noise:
 * stream 4 of (seed, utterance id) for a text row, streams 0-3 for a code row, so one utterance id may serve a refine stage and a code stage.
 * Log-probs of the code entry point (ctts_gpt_set_logprob_out) stay code-only: a text row writes none there; a text row's own log-probs are a separate opt-in,
 * ctts_gpt_set_text_logprob_out, after enable_text_rows.  A text row's adapter slot is an argument like any row's (admit_adapters).
 * Every ctts_gpt_begin switches the feature off again.  Under "batch_invariant" a text row's ids equal those of its batch-1 infer_text call bit for bit, and the
 * code rows' results do not depend on the text rows beside them.
 * Refused, each with a message: a mode-1 row without enable_text_rows; an engine without head_text / emb_text; use_penalty in text_sc; caller-supplied noise;
 * ctts_gpt_share_prompts groups of a call that seats a text row; ctts_gpt_restart while text rows are enabled (re-admit with attempt + 1); per-row sampling
 * knobs on a text row (set_row_sampling entries that differ from the call's values, admit_sampling entries); a call whose own infer_text is 1; text
 * max_new_token beyond the code call's. */
int ctts_gpt_enable_text_rows(ctts_gpt* h, const ctts_sampler_cfg* text_sc, int32_t* text_ids_dev, void* stream);
int ctts_gpt_set_row_modes(ctts_gpt* h, const int32_t* modes, int B);
int ctts_gpt_admit_modes(ctts_gpt* h, int n, const int32_t* rows, const int32_t* modes, void* stream);

/* Guided refine-text (no counterpart in the reference, whose refine pass samples freely over the 21178-way head and may drop, change or invent words): a GUIDE
 * makes a text row's output provably its source ids in order, with only ids of a small free set inserted, ended by EOS ([Ebreak]).  The state machine runs on the
 * device, inside the text sampler: the allowed set of a step depends on what the row drew one step earlier, and decode steps run as captured graphs.
 * Per call:       `free` = at most 64 distinct ids, each != eos and < vocab_text; max_run >= 0 = the most consecutive free ids allowed.
 * Per utterance:  src int32 [n], 1 <= n (at most 1020), n + 1 <= the row's limit, no id the EOS; device state cur (source ids emitted so far) and run (free ids
 *                 since the last source id), both starting at 0.
 * At the row's own step t, with limit L: need = n - cur, slack = (L - t) - (need + 1).
 *   Allowed set A   cur <  n:  A = {src[cur]}, plus `free` if run < max_run and slack > 0
 *                   cur == n:  A = {eos},      plus `free` if run < max_run and L - t > 1
 *   Arithmetic      elements outside A are treated exactly as elements j >= V are (not valid, -inf, before the division by the temperature); softmax, top-P,
 *                   top-K and the final race are the unguided arithmetic over A.  Only the <= 65 logits of A are loaded.
 *   min_new_token   removes EOS only while another element of A remains.
 *   Stand-in        when every race ratio is 0 or NaN (a NaN ratio counts as 0), the stand-in is src[cur] (EOS when cur == n), never id 0.
 *   Update          idx == src[cur] with cur < n: cur++, run = 0 (the source match takes precedence when src[cur] is also in `free`);
 *                   idx == eos: the row finishes; anything else: run++.
 *   Guarantees      a guided row always finishes by a sampled EOS within its limit (finish == 1); its ids are src with free ids interleaved; no run of free ids is
 *                   longer than max_run; it never ends at step 0, so ensure_non_empty never triggers on it.
 * The records are keyed by OUTPUT SLOT (the utterance's index in ids / finish / end_idx), like the log-prob buffers: compact, grow, cancel and admit need nothing
 * extra.  The table serves output slots 0..1023; the per-call block the sampler reads (SamplerDyn) holds its address, null = off.  Whether a step is guided is part
 * of the decode graphs' key.  Guided and unguided text rows may share a batch: a row whose slot has no record (n == 0) takes the unguided path, a test that is
 * uniform over its workgroup.  The unguided instantiation of the kernel is the kernel as it was.
 *   set_text_guide  the per-call part.  After ctts_gpt_begin of an infer_text call; for text rows in a code call after ctts_gpt_enable_text_rows.  Every slot
 *                   starts unguided.  Every ctts_gpt_begin (and ctts_gpt_enable_text_rows) switches the feature off again.
 *   set_guides      HOST out_slots [n], src_concat, src_off [n + 1]: the sources of the utterances at those output slots (entry i: src_concat[src_off[i] ..
 *                   src_off[i + 1])); a length of 0 = unguided.  Call it before the first sample, or before the ctts_gpt_admit that seats them; a slot that is
 *                   re-used gets a fresh record (cur = run = 0) -- name a re-used slot for its unguided successor too (length 0).  Asynchronous: the records go
 *                   through a pinned ring.  ctts_gpt_restart zeroes cur / run of the rows it restarts.
 * Refused, each with a message, before any launch: a free id equal to EOS, out of range or listed twice; more than 64 free ids; max_run < 0; a source id out of
 * range or equal to EOS; n + 1 > the row's limit (by set_guides for begin's rows, by ctts_gpt_admit for the rows it seats); an output slot >= 1024; caller-supplied
 * noise with guides in a code call; guides without the per-call part; a guide on a code row (set_text_guide in a code call without text rows; set_guides / admit on a
 * slot a code row holds).
 * Not offered: a gathered text head that computes only the logits of A (the head still streams its whole matrix); guides for code rows.  Log-probs of guided
 * (and unguided) text rows: ctts_gpt_set_text_logprob_out below. */
int ctts_gpt_set_text_guide(ctts_gpt* h, const int32_t* free_ids_host, int n_free, int max_run, void* stream);
int ctts_gpt_set_guides(ctts_gpt* h, int n, const int32_t* out_slots_host, const int32_t* src_concat_host, const int32_t* src_off_host, void* stream);

/* Shared prompt passes (no counterpart in the reference): sequences with ONE prompt -- the N candidates of an utterance, one text at several temperatures or
 * noise keys -- run it through the prompt pass once.  One-shot, like ctts_gpt_admit_sampling: names, for the NEXT ctts_gpt_begin (B == n) or ctts_gpt_admit
 * (its n == n), which prompt each sequence has.  prompt_of HOST [n], values in [0, n_prompts); every prompt named at least once.  While pending, the call's mask
 * is [n_prompts][T] and its emb (ctts_gpt_prefill / ctts_gpt_admit) is [n_prompts][T][hidden]: indexed by PROMPT, not by sequence; the prompt pass is
 * n_prompts x T rows high (n_prompts x (T - 1) under "batch_invariant" and in ctts_gpt_admit, whose fit check counts prompts).  The first sequence naming a
 * prompt (the leader) runs it through the prompt pass into its own KV lane; the others receive a copy of the prompt span of the lane and of the leader's pending
 * decode input (one launch after the last pass, kv_share.hip; never host-synchronised).  Every sequence keeps its own decode-row state: lane, utterance id,
 * limit, output index, sampling knobs; ctts_gpt_restart, ctts_gpt_compact and later admissions work as without the call.  Caller-supplied noise is allowed.
 * NULL / n == 0 clears.  Refused here: an index out of range, a prompt named by no sequence.  Refused by the begin / admit call that consumes the request (it is
 * consumed whether that call succeeds or fails): n differs from the call's; infer_text (code mode only); sequences of one group that carry different adapter
 * slots (ctts_gpt_set_row_adapters / ctts_gpt_admit_adapters) -- the prompt pass depends on the adapter, so a group shares one slot or none.
 * Without the call nothing changes: the same launches, bit-identical results. */
int ctts_gpt_share_prompts(ctts_gpt* h, int n, const int32_t* prompt_of_host, int n_prompts);

/* Log-probs of the sampled ids, written by the sampler as it draws them (no counterpart in the reference; ctts_gpt_score re-scores finished codes with a
 * prompt pass, and knows the raw heads only).  Per (utterance, step, codebook), for the id the sampler returned:
 *   lp_raw      log_softmax(raw logits)[id] -- the row as the code head wrote it, BEFORE the division by the temperature: the quantity ctts_gpt_score
 *               returns for the same token
 *   lp_sampled  log p(id) under the distribution the sampler drew from: the raw row after temperature, repetition penalty, top-P, top-K and the
 *               min_new_token rule, i.e. the log of the final softmax over the kept set at the chosen element.  When every ratio of the exponential race is
 *               0 or NaN, element 0 stands in for the draw and may lie outside the kept set: then lp_sampled is -inf
 * Both buffers are fp32 [n_out][max_new_token][4] device memory laid out like ctts_gen_io.ids (n_out = the extent of the ids array: indexed by the
 * utterance's output index, so ctts_gpt_compact and ctts_gpt_admit need nothing extra).  Either may be NULL (not wanted).  The values are stored next to
 * the id, under the id's condition (the row had not finished before the step):
 *   - the step that samples EOS IS written, at index end_idx (its ids are not part of the sequence, its log-probs are the probability of stopping there);
 *   - a finished row writes nothing; entries of steps a row never sampled keep the caller's fill (the call clears nothing);
 *   - an ensure_non_empty restart (ctts_gpt_restart, or re-admission with attempt + 1) overwrites from step 0.
 * Valid after ctts_gpt_begin and before the first ctts_gpt_sample / ctts_gpt_decode of the call.  Every ctts_gpt_begin resets both to NULL: callers that
 * never call this see no change -- the sampler then runs no extra reduction, and ids, hiddens, finish and end_idx are bit-identical with and without
 * log-probs (the values feed nothing back into the sampling arithmetic).  The two pointers live in the per-call device block the sampler reads, so captured
 * decode graphs are shared between calls with and without log-probs.  Under "batch_invariant" both values are part of the CONTRACT above: bit-identical
 * whatever the schedule.  Errors: no generate state (no begin, or ended by ctts_gpt_score), infer_text (the refine-text pass returns none), called after the
 * first sample. */
int ctts_gpt_set_logprob_out(ctts_gpt* h, float* lp_raw_dev, float* lp_sampled_dev, void* stream);

/* Log-probs of the refine-text pass: the text twin of ctts_gpt_set_logprob_out, a separate opt-in (the code entry point keeps refusing infer_text, and keeps
 * writing nothing for text rows).  Per (utterance, step), for the id the text sampler returned at the row's own step:
 *   lp_raw      log_softmax(raw text-head logits)[id] over the FULL vocab_text_head-wide row, before the division by the temperature -- for guided rows too (a
 *               guided row samples from its <= 65 allowed logits; for lp_raw it reads its whole row once more): the quantity ctts_gpt_score_text returns for
 *               the same token
 *   lp_sampled  log p(id) under the distribution the race drew from: logf(expf(x[id] - m2) * inv2) over the kept set, after temperature, guide mask, top-P,
 *               top-K and the min_new_token rule.  An id outside the kept set gives -inf: the unguided stand-in (element 0, when every ratio is 0 or NaN), a
 *               guided stand-in (src[cur] / EOS) that the warpers removed or whose probability underflowed to 0
 * Both buffers are fp32 [n_out][text max_new_token] device memory -- ONE value per step -- indexed by the utterance's output slot like the text ids (an infer_text
 * call: ctts_gen_io.ids' extent and the call's max_new_token; text rows in a code call: the extent of text_ids_dev and text_sc.max_new_token).  Either may be
 * NULL.  The values are stored next to the id, under the id's condition, with ctts_gpt_set_logprob_out's rules: the step that samples EOS is written at end_idx;
 * a finished row writes nothing; unsampled entries keep the caller's fill; a restart or a re-admission with attempt + 1 overwrites from step 0.  They feed nothing
 * back into the sampling arithmetic: ids, finish, end_idx and guide cursors are bit-identical with and without them, and a call that does not ask runs the same
 * launches.  The pointers live in the per-call block the text sampler reads (null = off; tests uniform over the workgroup), so captured decode graphs are shared
 * between calls with and without them.  One workgroup per row, fixed reduction order: under "batch_invariant" / "schedule_invariant" both values are part of the
 * CONTRACT.  Caller-supplied noise is allowed (an infer_text call): the values do not depend on where the noise comes from.
 * Valid after ctts_gpt_begin of an infer_text call, or after ctts_gpt_enable_text_rows in a code call, and before the first ctts_gpt_sample / ctts_gpt_decode;
 * begin and enable_text_rows reset both to NULL.  Refused by name: no generate state; a code call without text rows; a call after the first sample. */
int ctts_gpt_set_text_logprob_out(ctts_gpt* h, float* lp_raw_dev, float* lp_sampled_dev, void* stream);

/* Non-blocking variant: enqueues a copy of {steps_done, draws, all_finished, -} into 4 int32 of PINNED host memory; the
 * caller records an event after it and reads the words once the event has completed -- lets the host keep one chunk of
 * decode steps in flight while it inspects the previous one. */
int ctts_gpt_progress_enqueue(ctts_gpt* h, int32_t* host_pinned4, void* stream);

/* Test hooks (parity tests call the stages one by one through the same ABI):
 * logits of the current hidden rows fp32 [B][4][vocab_code] into `logits_dev` without sampling. */
int ctts_gpt_logits(ctts_gpt* h, float* logits_dev, void* stream);
/* force the next input token ids (teacher forcing): int32 [B][4] device; replaces the sampled ids and
 * re-embeds them (gpt.py:403-407). */
int ctts_gpt_force_ids(ctts_gpt* h, const int32_t* ids_dev, void* stream);
/* the Exp(1) noise the generate-mode sampler draws on the device (ctts_gen_io.noise == NULL) for one multinomial row:
 * out[j] = -log(u_j), u_j from Philox4x32-10 keyed by `seed`, counter (j | stream << 24, utterance id, step | attempt << 20); stream = codebook
 * 0..3, or 4 for the refine-text row.  fp32 [n] device.  Pinned by oracle/device_noise.py (tests/test_gpu_sampler.py). */
int ctts_sampler_noise(uint64_t seed, uint64_t utt_id, int stream_id, int step, int attempt, int n, float* out_dev, void* stream);
/* stand-alone sampler on caller-provided logits (fp32 [rows][vocab], rows = B*4; history int32
 * [rows][hist_len]; q fp32 [rows][vocab]) -> idx int32 [rows]; A15-A19 of SURVEY 8(a). */
int ctts_sampler_run(const ctts_sampler_cfg* sc, const float* logits_dev, const int32_t* history_dev, int hist_len,
                     const float* q_dev, int rows, int vocab, int step, int32_t* idx_dev, void* stream);
/* ... with knobs per sequence: row r uses per_seq[r / 4] (HOST [(rows + 3) / 4], <= CTTS_MAX_BATCH) instead of the knobs of `sc`; eos_token,
 * max_input_ids and max_new_token still come from `sc`.  The per-row path of the generate-mode sampler, stand-alone (a test hook). */
int ctts_sampler_run_rows(const ctts_sampler_cfg* sc, const ctts_row_sampling* per_seq, const float* logits_dev, const int32_t* history_dev,
                          int hist_len, const float* q_dev, int rows, int vocab, int step, int32_t* idx_dev, void* stream);

/* ... plus the log-probs of idx (ctts_gpt_set_logprob_out's definitions): lp_raw_out / lp_sampled_out fp32 [rows] device, either may be NULL. */
int ctts_sampler_run_rows_lp(const ctts_sampler_cfg* sc, const ctts_row_sampling* per_seq, const float* logits_dev, const int32_t* history_dev,
                             int hist_len, const float* q_dev, int rows, int vocab, int step, int32_t* idx_dev, float* lp_raw_out, float* lp_sampled_out,
                             void* stream);

/* Guided text sampler, stand-alone (a test hook, synchronous): ONE step of the generate-mode text kernel's guided instantiation -- the kernel itself, launched on
 * a one-step state the call builds -- on caller-supplied logits fp32 [rows][vocab] and noise q fp32 [rows][vocab] (device).  Row r carries the guide src_concat
 * [src_off[r] .. src_off[r + 1]) at cursor (cur[r], run[r]), at its own step[r] < limit[r]; all of these are HOST arrays, as are the results: the sampled id and the
 * cursor after the draw.  sc = the refine pass's parameters (infer_text = 1).  Refused by name: n == 0, n + 1 > limit, and everything ctts_gpt_set_text_guide /
 * ctts_gpt_set_guides refuse. */
int ctts_sampler_run_text_guided(const ctts_sampler_cfg* sc, const float* logits_dev, const float* q_dev, int rows, int vocab, const int32_t* free_ids_host, int n_free,
                                 int max_run, const int32_t* src_concat_host, const int32_t* src_off_host, const int32_t* cur_host, const int32_t* run_host,
                                 const int32_t* step_host, const int32_t* limit_host, int32_t* idx_out_host, int32_t* cur_out_host, int32_t* run_out_host, void* stream);

/* ... one step of the text kernel with the log-probs of the returned id (ctts_gpt_set_text_logprob_out's definitions; a test hook, synchronous).  src_concat_host
 * == NULL: unguided rows through the unguided instantiation (the guide arguments and cur_out / run_out are ignored and may be NULL); otherwise the guided one,
 * as above.  lp_raw_out_host / lp_sampled_out_host fp32 [rows], HOST; either may be NULL, both NULL = the launch of a call without the feature. */
int ctts_sampler_run_text_lp(const ctts_sampler_cfg* sc, const float* logits_dev, const float* q_dev, int rows, int vocab, const int32_t* free_ids_host, int n_free,
                             int max_run, const int32_t* src_concat_host, const int32_t* src_off_host, const int32_t* cur_host, const int32_t* run_host,
                             const int32_t* step_host, const int32_t* limit_host, int32_t* idx_out_host, int32_t* cur_out_host, int32_t* run_out_host,
                             float* lp_raw_out_host, float* lp_sampled_out_host, void* stream);

/* last measured average duration (ms) of one captured decode step, measured with hipEvents on the launch
 * stream around `n` graph replays; used by bench.py for the roofline object. */
int ctts_gpt_time_decode(ctts_gpt* h, int n_steps, float* ms_per_step, void* stream);

/* algorithmic bytes of one decode step at mean context L: s*(W + B*(L+1)*KV_tok). */
double ctts_gpt_step_bytes(const ctts_gpt* h, int B, double mean_ctx);

/* ------------------------------------------------------------------------------------------ */
/* DVAE decoder + Vocos (models/dvae.py decode branch; third-party vocos)                     */
/* ------------------------------------------------------------------------------------------ */

typedef struct ctts_voc ctts_voc;

typedef struct {
    int32_t dvae_idim;      /* 384 */
    int32_t dvae_hidden;    /* 512 */
    int32_t dvae_bn;        /* 128 */
    int32_t dvae_layers;    /* 12 */
    int32_t n_mels;         /* 100 */
    int32_t vocos_dim;      /* 512 */
    int32_t vocos_inter;    /* 1536 */
    int32_t vocos_layers;   /* 8 */
    int32_t n_fft;          /* 1024 */
    int32_t hop;            /* 256 */
    int32_t max_frames;     /* capacity in mel frames (2 per generated token) per utterance */
    int32_t max_batch;      /* utterances synthesised by one ctts_synth_batch call (<= 64) */
    /* optional quantiser of the DVAE_full model (configs/infer/chattts_plus.yaml dvae_encode.vq_config: G=2, R=2, levels 5,5,5,5):
     * vq_groups > 0 makes the handle a "decode codes" model (use_decoder=False, pipeline:292) -- dvae_idim = vq dim / G (512),
     * dvae_hidden 256; vq_groups == 0: the plain decoder (Decoder.pt) */
    int32_t vq_groups;
    int32_t vq_residuals;
    int32_t vq_levels[4];
} ctts_voc_cfg;

/* replaces DVAE.__init__ (dvae.py:203-239) + vocos.Vocos construction (pipeline:93-111) */
int ctts_voc_create(const ctts_voc_cfg* cfg, ctts_voc** out);
void ctts_voc_destroy(ctts_voc* h);
/* `name` = "dvae." + DVAE state-dict key  or  "vocos." + Vocos state-dict key; host fp32.  With vq_groups > 0 also
 * "dvae.vq_layer.quantizer.rvqs.{g}.project_out.{weight,bias}" (GroupedResidualFSQ, vector_quantize_pytorch). */
int ctts_voc_set_weight(ctts_voc* h, const char* name, const float* data, size_t numel);
int ctts_voc_finalize(ctts_voc* h);

/* DVAE.forward(mode="decode") (dvae.py:272-291): hidden fp32 [n][768] device (one utterance) ->
 * mel fp32 [100][2n] device.
 * Range (both calls below and the batched ones): the GEMMs keep fp32-level accuracy while their input activations lie in about
 * [2^-7, 65504] in magnitude; larger values (+-inf included) are clamped to +-65504, a row that is uniformly smaller loses accuracy
 * as 2^-25 / |x|, and NaN propagates to the output (it is not an error). */
int ctts_dvae_decode(ctts_voc* h, const float* hidden_dev, int n_tokens, float* mel_dev, void* stream);
/* vocos.Vocos.decode (pipeline:303): mel fp32 [100][F] device -> wav fp32 [hop*(F-1)] device */
int ctts_vocos_decode(ctts_voc* h, const float* mel_dev, int frames, float* wav_dev, void* stream);
/* the whole of ChatTTSPlusPipeline._decode_to_wavs (pipeline:286-305) for B utterances in one launch sequence:
 * hidden_ptrs[u] fp32 [n_tokens[u]][768] device -> wav_ptrs[u] fp32 [hop*(2*n_tokens[u]-1)] device; the two pointer
 * arrays and n_tokens are HOST arrays of length B (<= max_batch).  Same arithmetic as dvae_decode + vocos_decode. */
int ctts_synth_batch(ctts_voc* h, const float* const* hidden_ptrs, const int32_t* n_tokens, int B, float* const* wav_ptrs, void* stream);

/* use_decoder=False branch (pipeline:292,435-439: the DVAE_full model decodes the generated CODE IDS instead of the hidden states):
 * DVAE.forward decode with a quantiser (dvae.py:272-291) = GFSQ._embed (dvae.py:85-96: ids -> implicit FSQ codes, summed over the R
 * residual levels with scale (levels-1)^-r -> project_out, groups concatenated) + the same decoder stack.  Needs a handle created with
 * vq_groups > 0.  ids int32 [n][G*R] device (GPT.generate's ids rows, gpt.py:295-297) -> mel fp32 [100][2n]. */
int ctts_dvae_decode_codes(ctts_voc* h, const int32_t* ids_dev, int n_tokens, float* mel_dev, void* stream);
/* ... and _decode_to_wavs(result.ids, use_decoder=False) for B utterances in one launch sequence; ids_ptrs[u] int32 [n_tokens[u]][G*R]. */
int ctts_synth_batch_codes(ctts_voc* h, const int32_t* const* ids_ptrs, const int32_t* n_tokens, int B, float* const* wav_ptrs, void* stream);

/* Windows of the waveform (streaming; no counterpart in the reference, whose stream branch vocodes the whole prefix per chunk, pipeline:436-461).
 *
 * ctts_synth_window_range: host only, touches no GPU.  Tokens [a, b) whose vocoding contains samples [s0, s1) of the n_tokens-long prefix waveform exactly:
 * out5 = {a, b, sample offset of that sub-waveform (2 a hop), s0 clamped, s1 clamped}; an empty window gives five zeros.  A sample s depends on ISTFT frames
 * s/hop - 1 .. s/hop + 2, each on halo_frames - 3 mel frames either side; a token is two frames (halo_frames = 105 for the DVAE decoder + Vocos stack).
 *   clamp_tail != 0  a right edge inside the halo of the prefix's end is moved to the end: the zero padding there is part of the PREFIX waveform.  The window is
 *                    a slice of the n_tokens prefix's waveform, which later tokens change over its last halo.
 *   clamp_tail == 0  the rule for SETTLED windows: s1 <= hop * max(0, 2 n_tokens - halo_frames - 2), the samples no later token can change (every frame
 *                    the window needs exists: ceil(s1 / hop) + 1 + halo_frames + 1 <= 2 n_tokens); an unsettled s1 is an error.  b stays the unclamped
 *                    ceil(f1 / 2): the range does not depend on n_tokens, and the samples are those of the finished utterance.
 *
 * ctts_synth_windows: ctts_synth_batch / ctts_synth_batch_codes (codes != 0: src_ptrs[u] are int32 [n_tokens[u]][G*R] code ids, else fp32 [n_tokens[u]][768]
 * hidden rows) for B token sub-ranges, except that the last kernel overlap-adds only samples [skip[u], skip[u] + count[u]) of sub-waveform u and stores them at
 * element out_off[u] of ONE packed device buffer `out`: fmt 0 = float32 (bit-identical to the slice of ctts_synth_batch's output), fmt 1 = int16 PCM,
 * rintf(clamp(x, -1, 1) * 32767).  n_tokens, skip, count and out_off are HOST arrays of length B (<= max_batch); count[u] == 0 stores nothing; a window
 * outside its sub-waveform is refused.  Nothing else of `out` is written.  Like ctts_synth_batch it never synchronises the stream. */
int ctts_synth_window_range(int n_tokens, int64_t s0, int64_t s1, int hop, int halo_frames, int clamp_tail, int64_t* out5);
int ctts_synth_windows(ctts_voc* h, const void* const* src_ptrs, const int32_t* n_tokens, const int32_t* skip, const int32_t* count, int B, void* out,
                       const int32_t* out_off, int fmt, int codes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Zero-shot speaker prompt: waveform -> audio-prompt codes.
 * Replaces ChatTTSPlusPipeline.sample_audio_speaker (pipelines/chattts_plus_pipeline.py:279-284, called from :486-499) =
 * DVAE.forward(mode="encode") (models/dvae.py:263-270): MelSpectrogramFeatures (:171-199), / coef, downsample_conv
 * (:224-229), encoder = DVAEDecoder (:130-168), GFSQ (:66-126).  Weight names are the DVAE_full.pt state-dict keys
 * ("downsample_conv.*", "encoder.*", "vq_layer.quantizer.rvqs.{g}.project_in.*", "coef") plus two host-computed tables:
 * "mel.window" [n_fft] (periodic hann) and "mel.fb" [n_fft/2+1][n_mels] (torchaudio melscale_fbanks, htk, norm=None).
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct ctts_enc ctts_enc;
typedef struct {
    int32_t n_mels;        /* 100 */
    int32_t dim;           /* 512: downsample_conv width = encoder idim */
    int32_t enc_hidden;    /* 256 */
    int32_t enc_bn;        /* 128 */
    int32_t enc_layers;    /* 12  */
    int32_t enc_odim;      /* 1024 = vq dim */
    int32_t vq_groups;     /* G = 2 */
    int32_t vq_residuals;  /* R = 2 */
    int32_t n_fft;         /* 1024 */
    int32_t hop;           /* 256 */
    int32_t max_samples;   /* longest reference clip, in 24 kHz samples */
    int32_t pre_bound;     /* GroupedResidualFSQ release detail: 1 = residual starts from bound(project_in(x)) (1.17.8, see oracle) */
} ctts_enc_cfg;

int ctts_enc_create(const ctts_enc_cfg* cfg, ctts_enc** out);
void ctts_enc_destroy(ctts_enc* h);
int ctts_enc_set_weight(ctts_enc* h, const char* name, const float* host_data, size_t numel);
int ctts_enc_finalize(ctts_enc* h);
/* wav: n_samples fp32 on the device (mono, 24 kHz).  ids: int32 [G*R][T] on the device, T = ((1 + n_samples/hop) - 2)/2 + 1,
 * row g*R + r like GFSQ.forward's `ind` (dvae.py:108-113,126).  Optional test hooks (device, may be null):
 * mel_out [n_mels][F] = log-mel / coef, feat_out [T][enc_odim] = encoder output.
 * Non-finite audio (this call and the batched one): a NaN or +-inf sample is not an error.  Every mel frame whose 1024-sample window covers it is
 * NaN (the clip at 1e-5 keeps NaN, as torch.clip does), the other mel frames are untouched, and every (code frame, group) whose projected
 * features are not finite gets id -1 in all R rows -- never an id in [0, 625): the caller decides (the pipeline refuses the clip). */
int ctts_dvae_encode(ctts_enc* h, const float* wav, int n_samples, int32_t* ids, float* mel_out, float* feat_out, void* stream);
/* The same for B clips in one launch sequence (grid.z / grid.y = utterance, per-utterance frame and code counts from device tables uploaded
 * once per call): per batch it replaces B calls of sample_audio_speaker (pipelines/chattts_plus_pipeline.py:279-284) = B runs of
 * DVAE.forward(mode="encode") (models/dvae.py:263-270), which the reference can only loop over.  Like ctts_synth_batch the pointer arrays and
 * n_samples are HOST arrays of length B (1 <= B <= CTTS_ENC_MAX_BATCH) of device pointers: wav_ptrs[u] fp32 [n_samples[u]], ids_ptrs[u] int32
 * [G*R][T_u].  mel_ptrs / feat_ptrs (the test hooks of the single-clip call) may be null, and so may any entry of them.  Every output is
 * bit-identical to ctts_dvae_encode of that clip alone, whatever the batch, its order or its chunking.  All arguments are checked on the host
 * before the first launch: a clip outside (n_fft/2, max_samples] or a null wav / ids entry fails the call, its index in the message, and
 * nothing is written.  Workspace: a batch that fits the single-clip buffers (one clip of max_samples) uses them; the first batch that does
 * not allocates, once per handle, a second set 4 times as large (16 KiB per 256-sample frame of max_samples: about 180 MiB at 30 s, 360 MiB at 60 s) and every
 * batch is then served in as many chunks as fit it, each utterance region strided by its chunk's longest clip.  Never synchronises the stream
 * (but for that one allocation and, every fifth call in flight, the reuse of a pinned table slot). */
#define CTTS_ENC_MAX_BATCH 256
int ctts_dvae_encode_batch(ctts_enc* h, const float* const* wav_ptrs, const int32_t* n_samples, int B, int32_t* const* ids_ptrs,
                           float* const* mel_ptrs, float* const* feat_ptrs, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Output sample rate: torchaudio.functional.resample (sinc_interp_hann; the reference uses it on the input side, pipeline:495) as a device kernel for
 * the waveforms and streaming windows that LEAVE the engine.  A rate pair reduced by its gcd is orig : new_; width and the float32 table
 * kernels[new_][K], K = 2 width + orig, are audio.resample_kernels' (Python builds the table: libm's sin / cos are not torch's).  Output sample
 * j = i new_ + p of an n-sample waveform x is sum_k kernels[p][k] x[i orig - width + k], x = 0 outside [0, n); there are ceil(new_ n / orig) of them.
 *
 * Host-only geometry (no GPU), the twins of hip_models.resampler's functions:
 *   ctts_resample_out_total   ceil(new_ n / orig)
 *   ctts_resample_settled     output samples no later input can change once S input samples are settled: new_ max(0, floor((S - width) / orig)), every
 *                             output frame whose last tap lies below S; finished != 0: ctts_resample_out_total(n)
 *   ctts_resample_in_range    out2 = the inputs outputs [j0, j1) can read, before clipping to [0, n):
 *                             {(j0 / new_) orig - width, ((j1 - 1) / new_) orig + orig + width}; {0, 0} for an empty range
 *
 * ctts_resampler_create uploads the table once; a pair with K > CTTS_RESAMPLE_MAX_TAPS or a table above CTTS_RESAMPLE_MAX_TABLE_BYTES is refused.
 * ctts_resample_windows: ONE launch computes outputs [j0[u], j0[u] + count[u]) of B windows (1 <= B <= CTTS_RESAMPLE_MAX_WINDOWS, ragged, count 0
 * allowed) and stores them at element out_off[u] of `out`: fmt 0 = float32, fmt 1 = int16 PCM, rintf(clamp(y, -1, 1) * 32767).  src[u] is a device buffer
 * with input samples [src0[u], src0[u] + src_n[u]) of window u's waveform, total[u] the waveform's length or -1 while it is not known (an utterance still
 * decoding); the whole waveform is the window src0 = 0, total = src_n, j0 = 0, count = out_total.  All arrays are HOST arrays of length B, uploaded as one
 * pinned table per call.  Every argument is checked before the launch: in_range(j0, j0 + count) clipped to [0, total) must lie inside
 * [src0, src0 + src_n) (total = -1: its right edge must lie inside the buffer), else the call fails naming the window and nothing is written.
 * Each output is one ascending-k fmaf chain in float32 over all K taps, a tap outside [0, total) entering as an exact zero: its bits do not depend on
 * j0, src0, the tile it falls in or B, and equal the whole-waveform call's.  Never synchronises the stream (but for the reuse of a pinned slot). */
typedef struct ctts_resampler ctts_resampler;
#define CTTS_RESAMPLE_MAX_TAPS 1024
#define CTTS_RESAMPLE_MAX_TABLE_BYTES (4u << 20)
#define CTTS_RESAMPLE_MAX_WINDOWS 1024
int64_t ctts_resample_out_total(int orig, int new_, int64_t n);
int64_t ctts_resample_settled(int orig, int new_, int width, int64_t S, int finished, int64_t n);
int ctts_resample_in_range(int orig, int new_, int width, int64_t j0, int64_t j1, int64_t* out2);
int ctts_resampler_create(int orig, int new_, int width, const float* kernels_host, ctts_resampler** out);
void ctts_resampler_destroy(ctts_resampler* h);
int ctts_resampler_tile_frames(const ctts_resampler* h);      /* output frames per workgroup tile (tiles are counted from frame 0 of the waveform) */
int ctts_resample_windows(ctts_resampler* h, const float* const* src, const int64_t* src0, const int32_t* src_n, const int64_t* total,
                          const int64_t* j0, const int32_t* count, int B, void* out, const int64_t* out_off, int fmt, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTTS_HIP_H */
