// Host side of the GPT path: C ABI (include/ctts_hip.h), weight packing, launch sequencing, hipGraph.
//
// Layout in HBM (all owned by the handle unless noted):
//   packed weights   per layer  Wqkv [144 tiles][K=768]  Wo [48][768]  Wgu [384][768]  Wd [48][3072]
//                    + heads [157 tiles][768], each tile = 16 rows x KT cols stored [k-tile][lane][16 B]
//   KV cache         [layers][2][max_batch][heads][max_seq][64]   (caller-owned, bound with ctts_gpt_bind_kv)
//   residual stream  x_dec [B][768] fp32 (decode), x_pre [<= 16384 rows][768] (one prompt pass; sized min(16384, max_batch * max_seq))
//   act              fragment-major SwiGLU output for the down projection
//   xh / ssq / scale fp16 decode above the split-K batch sizes: the residual stream as packed fp16 B operand + per-tile sums of squares + per-row
//                    power-of-two scales, handed from the o_proj / down epilogues to the next QKV / gate|up / heads kernels (kernels.h PRO_XH)
//   lora_*           resident per-utterance adapters and the low-rank terms of the rows being processed (lora.hip)
//   dpart            [rows <= 32][4][768] ordered split-K partial sums of the down projection (decode batches <= split_rows)
//   st / dyn         DevState (per-step counters) and SamplerDyn (per-call buffers and sampling parameters): everything a captured
//                    decode graph would otherwise bake in is read from these two device blocks
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cmath>
#include <map>
#include <mutex>
#include <string>
#include <atomic>
#include <thread>
#include <vector>

#include "../../include/ctts_hip.h"
#include "kernels.h"
#include "persist.h"
#include "roctx_range.h"

static thread_local char g_err[512] = "";
void ctts_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* ctts_last_error(void) { return g_err; }
extern "C" int ctts_version(void) { return 1; }

#define PASS_ROWS_MAX 16384   // prompt rows per pass (32 x 512 tokens in one pass); an engine's workspaces are sized for min(this, max_batch * max_seq)
#define PASS_PAD 256          // + PASS_PAD rows so that whole GEMM blocks stay in bounds
#define SMAX 8        // == ATT_SMAX in skinny_gemm.hip
#define CTTS_PERSIST_MAX_ROWS PL_MAXR

struct DecodePath { int splits, persist; };      // how a decode step runs: key splits of the decode attention (decode_splits) / key shares of the persistent launch, 0 = the launch chain (decode_persist)
struct LayerW {
    void *qkv, *o, *gu, *d;      // RMSNorm weights are folded into qkv / gu columns
    // fp32 engines: head / tail fp16 images of 64 * W, [tile][k tile][head | tail][lane][16 B] in the fp16 tile order (common.h split_t): the prompt pass's split
    // GEMMs (prefill_split.hip) and the decode projections from split_decode_rows rows on (skinny_gemm.hip) read them
    void *qkv_sp = nullptr, *o_sp = nullptr, *gu_sp = nullptr, *d_sp = nullptr;
};

// The host's record of one decode row -- a new per-row property joins this struct: KV lane; context length (an upper bound: advance_rows) and its cap, prompt + token limit;
// 0 code / 1 text (RowState.mode); adapter slot or -1 as the decode launches carry it (row_slot_bytes; the prompt pass reads the lane table lora_slot_host)
struct HostRow { int seq, ctx, cap, mode, slot; };
// What the callers asked for ahead of a call.  RowRequests persist ("the following begin calls", until set again); a NextCall is for the next ctts_gpt_begin / ctts_gpt_admit alone
struct RowRequests {
    std::vector<RowSampling> knobs;              // ctts_gpt_set_row_sampling, per sequence (empty = the call's values); checked by begin, against that call's max_new_token
    std::vector<int> modes;                      // ctts_gpt_set_row_modes, per sequence
    std::vector<int> slots;                      // ctts_gpt_set_row_adapters, per KV lane [CTTS_MAX_B]: every begin() / score() starts from it again, whatever the previous call did to the live tables
};
struct NextCall {
    std::vector<int> share; int share_P = 0;     // ctts_gpt_share_prompts: prompt of every sequence of the call (empty = none) and the number of prompts
    std::vector<std::pair<int, RowSampling>> knobs;   // ctts_gpt_admit_sampling: (row, knobs) of the utterances the admission seats
    std::vector<std::pair<int, int>> modes;      // ctts_gpt_admit_modes: (row, mode) of the same
};

struct ctts_gpt {
    ctts_gpt_cfg cfg;
    int H, I, NH, L, V, NVQ;
    int esz;                                     // element size of weights / KV
    std::map<std::string, std::vector<float>> host;   // staged fp32 weights until finalize
    bool finalized = false;
    // device
    char* wblob = nullptr;
    char* wsplit = nullptr;                      // fp32 engines: the split images of every layer matrix (2 x 2 bytes per weight), or null
    void* whead_sp = nullptr;                    //   ... and of the folded code heads
    bool split_ok = false;                       //   every weight x 64 is inside the fp16 range (otherwise the engine stays on the exact fp32 kernels)
    int split_nbg2_rows = 17;                    // ... and from this many rows on they take 32-row blocks (one workgroup per weight tile streams it once for all 32 rows; the down projection's K is
                                                 // sliced four ways inside the launch as at 16-row chunks).  ms/step 16-row chunks / 32-row blocks: 17 rows 0.723 / 0.700, 24: 0.822 / 0.800, 32: 0.846 / 0.824
                                                 // (profiles/r06_ab_split_shapes.jsonl).  "split_nbg2_rows"
    int prefetch_kb = 96;                        // decode launch chain, packed-residual path (>= 9 rows; fp16 engines: >= 17): the o_proj launch -- 2.4 MB of weights of its own -- carries extra
                                                 // workgroups that pull the gate|up launch's 18.9 MB weight image into L2 (kernels.h WPrefetch), one per this many KiB of it (8..256 of
                                                 // them); 0 = off.  "weight_prefetch_kb".  ms/step without / with (profiles/r06_ab_weight_prefetch.jsonl): fp32 batch 9 0.610 / 0.588, 16 0.635 / 0.605,
                                                 // 32 0.826 / 0.804; fp16 batch 32 0.603 / 0.588.  The other carriers stream large matrices themselves and lose what their consumers gain
                                                 // (down carried by gate|up +4.8 %, the next q|k|v carried by down +2.7 %), and at 6-8 rows (split-K launch slices) the o_proj carrier loses
                                                 // too: off there.  The role is compiled into that one launch only: present in a kernel it costs 0.3 us per launch even when unused
    int split_dec_rows = 9;                      // fp32 engines: decode batches of >= this many rows (packed-residual path, no per-utterance adapters) run their projections on the
                                                 // head / tail images: 3 fp16 MFMAs per product instead of 8 exact-f32 ones (skinny_gemm.hip dispatch_split); 0 = never.  "split_decode_rows"
    void *sp_x_hi = nullptr, *sp_x_lo = nullptr, *sp_act_hi = nullptr, *sp_act_lo = nullptr;   //   ... and of the prompt rows' operands
    int split_rows_min = 65;                     //   prompt passes of at least this many rows use them.  384 until the end of round 6 (prompt pass ms row kernels / split GEMMs then:
                                                 //   192 rows 2.0 / 3.0, 384 rows 3.1 / 3.0, 768 rows 5.3 / 3.6); with 64 x 64 blocks and the sliced down projection of short
                                                 //   passes (prefill_split.hip sp_launch) the split GEMMs win from the first pass that has more than one 64-row block:
                                                 //   66 rows 1.48 / 1.22, 96: 1.52 / 1.23, 192: 2.13 / 1.31, 288: 2.58 / 1.39, 360: 3.24 / 1.60 (diagnostic builds: CTTS_PREFILL_SPLIT, 0 = never)
    std::vector<LayerW> lw;
    void* whead = nullptr;
    void* whead_text = nullptr;                  // refine-text head (21178 x H), packed like whead; optional
    // text rows beside code rows in one decode batch (ctts_gpt_enable_text_rows; RowState.mode): the mode is a property of the ROW (HostRow.mode), the call stays a code-mode call
    SamplerCfgDev sc_text = {};                  //   the text rows' sampling parameters (the refine pass's ctts_sampler_cfg)
    SamplerDyn* dyn_text = nullptr;              //   device: the text block -- sc_text, the text ids array, and the code block's finish / end_idx / seed
    float* logits_text = nullptr;                //   [max_batch][vocab_text_head]; both allocated by the first ctts_gpt_enable_text_rows
    float* lnf = nullptr;
    float* emb_code = nullptr;
    float* emb_text = nullptr;                   // [V_text][H] prompt embedding table (optional)
    int vocab_text = 0;
    int vocab_text_head = 0;
    float* rope = nullptr;
    float *rope_pre = nullptr, *rope_dec = nullptr;   // per-row copies of the table rows (prefill rows / decode rows)
    int rope_n = 0;
    char* kv = nullptr;
    size_t kv_bytes = 0;
    float* sk_scratch = nullptr; size_t sk_cap_floats = 0;      // split-K partial outputs of short prompt passes (finalize)
    float *x_dec = nullptr, *x_last = nullptr, *x_pre = nullptr, *q_buf = nullptr, *part_ml = nullptr, *part_o = nullptr, *logits = nullptr;
    void* act = nullptr;
    void* attn_packed = nullptr;
    void* norm_packed = nullptr;                 // prompt pass: RMSNorm'ed rows in the GEMMs' fragment-major operand layout (norm_pack_kernel)
    int split_rows = 4;                          // decode batches up to this size run the down projection as 4 split-K launch slices whose
                                                 // partial sums the next consumers add (0 = off): 48 x 1024-thread blocks -> 192 x 256/512.
                                                 // fp16: 8 (us/step with the threshold at 4 / 16: batch 5 474 / 458, 8 477 / 470, 16 515 / 585 -- above 8 the
                                                 // packed-fp16 residual hand-off wins); fp32: 16 = every single-chunk batch (batch 5 633 -> 572, 8 674 -> 612,
                                                 // 16 766 -> 712: 48 blocks pulling 9.4 MB of fp32 weights + as many bytes of fp32 activations through 48 CUs were
                                                 // the slowest launch of the layer; with two 16-row chunks the partial sums cost the next QKV prologue what the
                                                 // split saves: batch 20 / 24 / 28 / 32 835 / 892 / 914 / 941 either way)
                                                 // Round 4: fp32 8 as well -- with the in-launch split-K combine (down_sk_rows) the packed-residual path wins from 9 rows on:
                                                 // ms/step launch slices / packed + combine: batch 8 0.599 / 0.613, 9 0.632 / 0.623, 10 0.641 / 0.627, 12 0.664 / 0.637,
                                                 // 14 0.687 / 0.648, 16 0.709 / 0.661; launch slices beyond 16 rows lose (17 0.765 -> 0.812, 32 0.860 -> 0.939)
    float* dpart = nullptr;                      // [rows<=32][4][768]
    int launched = 0;                            // decode steps enqueued since begin / restart: host-side bound on the context length
    int nbg2_rows = 33;                          // decode batches of at least this many rows use 32-row blocks instead of 16-row chunks.
                                                 // Measured: two 16-row chunks beat one 32-row block at batch 24 / 32 (598 vs 624,
                                                 // 640 vs 660 us/step) -- per-block prologue latency, not L2 traffic, is what these launches pay for;
                                                 // the prompt pass keeps 32-row blocks
                                                 // Round 4 (with the in-launch split-K combine of the 16-row chunks): ms/step 32-row blocks / 16-row chunks, fp32: batch 40 1.176 / 1.012,
                                                 // 48 1.266 / 1.100, 64 1.343 / 1.259, 96 1.717 / 1.754, 128 2.081 / 2.159; fp16: 40 0.676 / 0.652, 64 0.767 / 0.768, 128 1.099 / 1.169
                                                 // -> 32-row blocks from 81 (fp32) / 57 (fp16) rows ("nbg2_rows")
    int force_splits = 0;                        // key splits of the decode attention (0 = decode_splits policy); ctts_gpt_set_option("decode_splits")
    int down_sk_rows = 9;                        // xh-mode decode batches of >= this many rows (one 16-row chunk per block) slice the down projection's K four ways inside the
                                                 // launch (EPI_RESID_XH_SK); 0 = never.  "down_splitk_rows".  us/step without -> with (profiles/r04_ab_down_splitk.jsonl):
                                                 // fp32 batch 17 795 -> 767, 24 862 -> 833, 32 894 -> 868; fp16 batch 9 475 -> 465, 16 507 -> 496, 24 / 32 unchanged
    float* sk_slab = nullptr; int* sk_cnt = nullptr;
    int opt_gen = 0;                             // bumped by ctts_gpt_set_option: part of the decode-graph key
    int graph_gen = 0;                           //   the opt_gen the cached graphs were captured under: graphs of an older generation can never be selected again and are dropped
    int valu_rows = 2;                           // fp32 engines: decode batches of <= this many rows multiply on the VALU (skinny_gemm.hip, VR template argument):
                                                 // an exact-f32 MFMA costs 32 cycles whatever the number of live columns, 48 of them per SIMD and launch.
                                                 // Measured (us/step, MFMA -> VALU, profiles/r04_ab_valu_rows.jsonl): batch 1 481.9 -> 450.8, 2 491.7 -> 477.5,
                                                 // 3 532.6 -> 555.9, 4 536.7 -> 560.3 (the 4-row variant re-reads four LDS operand rows per weight fragment)
    int persist_rows = 0;                        // default 8 (fp32) / 5 (fp16), set at create: decode batches of <= this many rows run the decoder stack as ONE persistent
                                                 // launch (persist_layer.hip).  us/step, launch chain -> persistent (profiles/r04_ab_persist_options.jsonl):
                                                 // batch 1 452 -> 285, batch 2 480 -> 347, batch 4 540 -> 467
    bool persist_ok = false;                     //   the mode's preconditions hold and this process holds the device's lock (ensure_persist)
    char* pimg = nullptr;                        //   per-workgroup register images of the layer weights [L][192][192 KB], built on the device from the packed tiles -- on the FIRST
                                                 //   decode call of <= persistent_rows rows (persist_images): an engine that only ever decodes larger batches (a LoRA-merged
                                                 //   sibling serving batch 32) never pays the second 755 MB weight copy
    char* pimg_head = nullptr;                   //   the folded heads as 14 register-fragment rows per GEMV workgroup (persist.h PL_HEAD_FRAGS): the launch that ends the stack also runs
    int persist_delay_u = -1;                    //   "persistent_delay_lora": poll delay of the u granules, -1 = 14 + 2 rows (ms/step with an adapter on every row, delay 0 / 8 / 16 / 24:
                                                 //   batch 1 0.362 / 0.350 / 0.301 / 0.315, 2: 0.417 / 0.410 / 0.349 / 0.353, 4: 0.486 / 0.513 / 0.441 / 0.430; profiles/r06_ab_lora_persistent.jsonl)
    int prefill_pp_blocks = 1;                   // "prefill_pp_blocks": a split GEMM of the prompt pass may run on prefill_split_gemm_pp_kernel (256-row blocks, counter-phased wave groups) when it has
                                                 //   at least this many such blocks and the round count favours it (prefill_split.hip sp_launch); 0 = never
    int prefill_small_blocks = 192;              // "prefill_small_blocks": prompt-pass split GEMMs of at most this many 128 x 128 blocks (K slices counted) run on 64 x 64 blocks (0 = never)
    int prefill_ring4_blocks = 256;              // "prefill_ring4_blocks": prompt-pass split GEMMs of at most this many 128 x 128 blocks run with a 4-stage LDS ring, one block per CU (0 = never)
    int prefill_sk_rows = 2048;                  // "prefill_splitk_rows": prompt passes of <= this many rows slice the down projection's K four ways (prefill_split.hip sp_launch; 0 = never)
    int attn_wide_blocks = 0;                    // "attn_wide_blocks": decode attention takes 8-wave blocks while rows x heads < this (0 = 256).  Set at create: 512 (fp32) / 4096 (fp16).
                                                 //   Until round 6 the limit was one block per CU (256), tuned on the round-4 attention layout; on the V-one-dim-per-lane layout
                                                 //   8-wave blocks win further up (ms/step 4-wave / 8-wave, fp32: 22 rows 0.749 / 0.724, 28: 0.773 / 0.749, 32: 0.785 / 0.768, 40: 0.946 / 0.939,
                                                 //   48: 1.010 / 1.032; fp16: 32 rows 0.574 / 0.567, 48: 0.683 / 0.668, 64: 0.740 / 0.713; profiles/r06_ab_attn_wide_blocks.jsonl) --
                                                 //   this was round 5's unexplained 20 -> 22-row step (+10 %)
    int persist_share_keys = 384;                //   "persistent_share_keys": keys per key share at 1..5 rows; one share serves up to this + 128 keys (384 in registers, the rest -- up to 256 -- waits in LDS
                                                 //   since round 6 instead of streaming behind the query), more keys open a second share.  Re-swept with the LDS tail: 384 stays the best or ties
                                                 //   from 400 to 1000 keys (one share of 640: context 630 0.279 vs 0.263 ms/step with two shares; profiles/r06_ab_pair_lds_tail.jsonl)
    int persist_lora = 1;                        //   "persistent_lora": rows with per-utterance adapters stay on the persistent launch (round 6; 0 = they take the launch chain, as until round 5).  q/k/v/o terms only: rows whose adapter names an MLP target take the chain (lora_mlp)
    int persist_heads = 1;                       //   the final RMSNorm + heads ("persistent_heads"; code mode, paced schedule): one launch fewer per step
    unsigned long long* pl_g = nullptr;          //   granule buffers g_qkv | g_att | g_x1 | g_act
    unsigned* pl_epoch = nullptr;                //   launch counter = granule tag
    int* pl_error = nullptr;                     //   first give-up code (0 = none); reported by ctts_gpt_progress
    unsigned long long* pl_ts = nullptr;         //   diagnostics: per-workgroup phase marks of the last launch ("persistent_timestamps")
    int pl_ts_on = 0;
    int persist_fault = 0;                       //   test hook ("persistent_fault"): see PersistArgs.fault
    int persist_pair_keys = 704;                 //   6..8 rows: contexts beyond this many keys (minus 128 per row above 6) go back to the launch chain; "persistent_pair_keys"
    int persist_splits = 0;                      //   cap on the attention's key splits per (row, head) (0 = PL_SMAX); "persistent_splits"
    int persist_max_keys = 0;                    //   contexts beyond this many keys go back to the launch chain (0 = no limit); "persistent_max_keys"
    int persist_lpl = 0;                         //   decoder layers per persistent launch (0 = all of them in one launch)
    int persist_sched = 3;                       //   weight request schedule (PersistArgs.sched): 1 and 2 measure the same (389.3 / 389.5 us at batch 1, 436.0 / 436.4 at 2);
                                                 //   3 = paced requests: batch 1 373.0 -> 337.4, 2 425.7 -> 404.0, 3 490.1 -> 467.6 (profiles/r04_ab_persist_options.jsonl)
    int persist_pace = -1;                       //   -1 = by row count: 3 at 1-2 rows, 2 from 3 rows on (round 5, after the joint row sums: ms/step at pace 2 / 3, batch 1: 0.2377 / 0.2342,
                                                 //   2: 0.2747 / 0.2722, 3: 0.3190 / 0.3221, 4: 0.3489 / 0.3574, 5: 0.4066 / 0.4136).  Round 4 on PersistArgs.pace (us/step at batch 1 before the poll delays: 0 -> 356, 2 -> 342, 3 -> 337.5, 4 -> 339, 6 -> 341, 8 -> 354.6; with them 2 / 3 / 4 / 6: 285.0 / 286.6 / 293.0 / 297.7)
    // ~128-cycle units an edge wave sleeps before its first poll of the (x + attention) / act / layer-output edge: a pass that starts before the producers'
    // stores are visible fails and costs a whole extra pass, and its loads sit in the queues of the very stores it waits for.  us/step at batch 1 with all three at
    // 0 / 6 / 10 / 14 / 18 / 24 / 32: 334.9 / 307.6 / 288.8 / 281.6 / 286.5 / 295.9 / 316.3; batch 2 at 0 / 12: 402.3 / 346.9; batch 4: 521.2 / 467.4.
    // One at a time around 14 each curve is flat from 11 to 17 (profiles/r04_ab_persist_options.jsonl).  The attention edge needs none (its wait is long).
    // Round 5, after the attention workgroups' phase went from 1.9 to 1.25 us (tools/sweep_persist_delays.sh, ms/step at batch 1 | 4): attention edge 0 / 4 / 8:
    // 0.2457 / 0.2456 / 0.2456 | 0.4088 / 0.4044 / 0.4033; act edge 12 / 14 / 16 / 18 / 20: 0.2409 / 0.2402 / 0.2425 / 0.2430 / 0.2436 | 0.4165 / 0.4136 / 0.4125 /
    // 0.4117 / 0.4113 -> 14 + 2 per further row; the other two stayed where they were (10-12 and 13-15).
    int persist_delay_att = 8, persist_delay = 12, persist_delay_act = 14, persist_delay_x = 15, persist_nap = 1, persist_nap_qkv = 1;
    int persist_poll = -1;                       //   PersistArgs.poll; -1 = by row count: the sentinel pass costs one serial poll at 1-2 rows (batch 1 379.2 -> 387.1 us,
                                                 //   batch 2 430.7 -> 437.8) and pays from 3 rows on, where a full sweep re-reads up to 96 granules per lane (batch 4 547.5 -> 537.6)
    int no_prepack = 0, prefill_gemm_rows = 1536, xh_heads = 1;   // diagnostic builds only: see run_layers / run_decode_step
    int batch_inv = 0;                           // "batch_invariant" (fp32 engines): one arithmetic per row whatever the schedule (include/ctts_hip.h states the contract).  Decode: the split
                                                 //   projections on 16-row chunks at every row count, the down projection's K always sliced in the launch, layer 0 and the heads in one form, unsplit
                                                 //   8-wave attention, no persistent launch, no VALU rows.  Prompt: the split GEMMs at every pass height, K never sliced, attention chunks anchored
                                                 //   at the first real key.  begin: the last prompt token runs through the first decode step's layer pass, as after ctts_gpt_admit
                                                 //   fp16 engines take the same contract as "schedule_invariant" (this field under its dtype-independent name; on fp32 engines a synonym): the launch chain on the
                                                 //   packed fp16 residual stream in 16-row chunks at every row count with the same pins, and ONE prompt arithmetic -- norm_pack + the prefill_gemm.hip GEMM on
                                                 //   128 x 128 blocks at every pass height, the MFMA flash attention anchored at the first real key -- instead of the split GEMMs (plan_layers, inv16)
    float* rope_dec0 = nullptr;                  //   ... the decode rows' RoPE rows at begin (ctts_gpt_restart replays the first layer pass)
    RowMeta *meta_pre = nullptr, *meta_dec = nullptr, *meta_dec0 = nullptr;
    DevState* st = nullptr;
    int* last_rows = nullptr;
    int* host_pin = nullptr;
    // per-utterance LoRA (lora.hip): resident adapters A [layer][slot][target][16][768] and B^T in the same shape (zero padded to r = 16),
    // per-sequence slot table, low-rank terms of the rows being processed
    float *lora_A = nullptr, *lora_B = nullptr, *lora_scale = nullptr, *ln1 = nullptr;
    float* lora_Af = nullptr;                    //   A of q | k | v with the input RMSNorm weight folded into the columns [layer][slot][3][16][768]: the persistent launch's waves read it (persist_layer.hip LORA)
    std::vector<float> ln1_host;                 //   host copy of ln1 (fetched at the first ctts_gpt_set_adapter)
    int* lora_slot_of_seq = nullptr;
    std::vector<signed char> lora_rank;          //   [layer][slot][target] rank as loaded (0 = empty)
    std::vector<int> lora_slot_host;             //   host copy of lora_slot_of_seq, per KV lane (the decode ROWS' slots: HostRow.slot)
    float *lora_dqkv = nullptr, *lora_do = nullptr;
    unsigned long long* lora_g = nullptr;        //   decode steps: the same terms as tagged granules from worker workgroups inside the QKV / o_proj launches (lora_worker.h)
    int lora_fold = 1;                           //   "lora_fold" option: 0 = the two extra launches per layer at decode too
    // ... on the MLP projections (gate_proj / up_proj / down_proj): tables of their own, allocated when the first such target is loaded (737 KB per layer and slot;
    // engines that serve q/k/v/o adapters keep their footprint): A_gu [layer][slot][gate | up][16][768], B_gu [layer][slot][gate | up][16][3072],
    // A_d [layer][slot][16][3072], B_d [layer][slot][16][768] (rank-major, zero padded to r = 16), scale [layer][slot][4] = gate, up, down, -
    float *lora_mA_gu = nullptr, *lora_mB_gu = nullptr, *lora_mA_d = nullptr, *lora_mB_d = nullptr, *lora_mscale = nullptr, *ln2 = nullptr;
    float* lora_dgu = nullptr;                   //   gate / up terms of the rows being processed [rows][gate | up][3072] (the down term shares lora_do: o_proj has consumed it by then)
    std::vector<signed char> lora_mrank;         //   [layer][slot][gate, up, down] rank as loaded (0 = empty; sized last: non-empty = the tables above are all there)
    std::vector<float> ln2_host;                 //   post_attention_layernorm weights [layer][768], kept from finalize (61 KB): engines without MLP adapters allocate what they always did
    int pass_rows = PASS_ROWS_MAX;               // prompt rows per pass of this engine (env CTTS_PASS_ROWS, read once at finalize, lowers it: the
                                                 // one capacity knob of the product library; the multi-pass tests use it)
    void* xh = nullptr;                          // fp16 decode, > split_rows rows: residual stream as packed fp16 B operand (EPI_RESID_XH -> PRO_XH)
    float *ssq = nullptr, *scale_o = nullptr, *scale_d = nullptr;   //   per-tile sums of squares [rows][48]; per-row power-of-two scales of the xh rows
    int xh_mode = 1;                             //   0 (diagnostic builds) switches the path off (every block re-normalises fp32 rows: PRO_NORM)
    int* sat = nullptr;                          // fp16 engines: saturated / NaN fp16 stores since begin (common.h sat_half; ctts_gpt_saturations)
    int* hist_ring = nullptr;                    // sampler: repetition-penalty window ring [max_B][4][16] (sampler.hip)
    RowState* finend = nullptr;                  // sampler: per-row state [max_B] (common.h): mirror of {finish, end_idx}, noise key, token limit
    std::vector<RowState> finend_host;           //   its initial image for the current generate() (uploaded by begin)
    RowSampling* knobs = nullptr;                // sampler: per-row sampling knobs [max_B] (common.h), in the same allocation right behind finend (fixed address: the
                                                 //   captured graphs hold no per-call state)
    RowSampling* cknobs = nullptr;               //   compaction gather target / staging of the knobs an admission seats
    std::vector<RowSampling> knobs_host;         //   begin's image of rows 0..B-1
    // finished-row compaction (ctts_gpt_compact): gather targets + the kept row indices
    float *cx = nullptr, *crope = nullptr; RowMeta* cmeta = nullptr; int* cring = nullptr; RowState* cfin = nullptr; int* keep_dev = nullptr;
    std::vector<int> keep_host;
    std::vector<RowState> fresh_host;
    std::vector<int> seq_host;
    hipStream_t cap_stream = nullptr;
    SamplerDyn* dyn = nullptr;                   // device copy of the per-call sampler state (rewritten by begin; read by the heads + sampler nodes)
    // Captured decode graphs, keyed by what shapes the launches (batch, mode, KV binding): caller buffers and sampling
    // parameters are read from `dyn` at run time, so consecutive generate() calls replay the same executable graph.
    struct GraphEntry { hipGraph_t graph; hipGraphExec_t exec; };
    std::map<std::string, GraphEntry> graphs;
    hipGraphExec_t gexec = nullptr;              // entry selected by the last ensure_graph
    int graph_steps = 4;                         // decode steps captured per graph: a replay costs ~8 us of
                                                 // GPU-side gap, amortised over 4 x 102 kernel nodes
    int graph_steps_persist = 16;                // ... and per graph of the persistent paths (2 nodes per step: 32 nodes): the replay gap is 8.1 us whatever the graph
                                                 // holds (profiles/r05_trace_gaps_b1.json), 2.0 us per step at 4 steps, 0.5 us at 16
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // scoring scratch (score_rows), one per head, each allocated by its head's first call (engines that never score, or never score text, keep their footprint):
    // the gathered scored rows [chunk][H], their head logits [chunk][logits width] and output entries [chunk]
    struct ScoreScratch { float *x = nullptr, *logits = nullptr; int* oidx = nullptr; };
    ScoreScratch score_code;                     // ctts_gpt_score: chunk = SCORE_ROWS, 4 * V wide
    ScoreScratch score_text;                     // ctts_gpt_score_text: chunk = min(max_batch, SCORE_ROWS) ("score_text_chunk"), vocab_text_head wide (at most 128 x 21178 fp32 = 10.8 MB)
    int score_text_chunk = 0;
    // shared prompt passes (ctts_gpt_share_prompts; kv_share.hip)
    std::vector<int> share_tab;                  //   host image of share_dev for the call that consumed the request (kernels.h SH_*)
    int* share_dev = nullptr;                    //   device table [SH_INTS], allocated by the first ctts_gpt_share_prompts
    // guided refine-text (kernels.h GuideTab): the table is allocated by the first ctts_gpt_set_text_guide (4.2 MB; engines that never call it keep their footprint),
    // the records are uploaded through a pinned ring (a slot is reused only after its copies have run)
    GuideTab* guide_tab = nullptr;
    std::vector<int> guide_len;                  //   host mirror of rec[slot].n for the current call
    int* guide_pin = nullptr;
    hipEvent_t guide_ev[4] = {};
    bool guide_pin_used[4] = {};
    unsigned guide_pin_next = 0;
    std::vector<void*> owned;                    // every device buffer of the engine (dev_alloc)
    RowRequests req;                             // what the callers asked for: "the following begin calls"
    NextCall next;                               //   ... and the next ctts_gpt_begin / ctts_gpt_admit alone
    // ---- the current generate state: what ctts_gpt_begin starts and ctts_gpt_score ends (end_generate_state) ----
    int B = 0, T = 0, B0 = 0;                    // rows in the decode batch (0 = no generate state), prompt tokens per sequence and sequences at begin
    std::vector<HostRow> rows;                   // one record per decode row: size == B whenever a generate state exists
    SamplerCfgDev sc; ctts_gen_io io = {};       // the call's sampling parameters and buffers
    bool admitted = false;                       // ctts_gpt_admit / ctts_gpt_grow changed the rows of this generate(): x_last / meta_dec0 no longer describe them
    bool sampled = false;                        // a sample phase has been enqueued since begin (ctts_gpt_set_logprob_out is refused from then on)
    struct DecodeSeg { int n; DecodePath path; };
    std::vector<DecodeSeg> segs;                 // plan_decode: the steps of one decode call as runs of equal decode paths
    int share_P = 0, share_groups = 0;           // prompts of the current ctts_gpt_begin (0 = every sequence runs its own prompt; read by ctts_gpt_prefill), those with at least one follower
    long pp_rows = 0; int pp_T = 0;              // the last ctts_gpt_prefill / ctts_gpt_score call: its prompt rows and their tokens per sequence (debug_read "prompt_plan", "meta_pre", "x_pre"); 0 rows = none since begin
    int text_mode = 0, text_rows_on = 0;         // the call's own infer_text; the state has its text block (ctts_gpt_enable_text_rows; begin switches it off again)
    int guide_on = 0;                            // guided refine-text (ctts_gpt_set_text_guide): the text sampler runs its GUIDED instantiation -- part of the graph key; begin switches it off again
    // ... and what refresh_rows derives from `rows`: which launches a step takes is decided from these
    int text_live = 0;                           // rows whose mode is 1, finished ones included ("text_rows_live"): > 0 = the step is MIXED -- two more launches (text head, text sampler)
    int lora_rows = 0;                           // 1: a row carries an adapter slot; before rows exist (ctts_gpt_set_row_adapters, ctts_gpt_score) the sequences of the request do
    int lora_mlp = 0;                            // 1: such a slot holds an MLP target ("lora_mlp_live"): two more launches per layer, decode on the launch chain at every row count
};
#define SCORE_ROWS 2048       // scored rows per heads launch: bounds the logits scratch (2048 x 2504 fp32 = 20.5 MB)

// Device buffers belong to the engine: every allocation is recorded, ctts_gpt_destroy frees what is on the record
static int dev_alloc(ctts_gpt* h, void** p, size_t bytes) {
    CTTS_HIP_CHECK(hipMalloc(p, bytes));
    h->owned.push_back(*p);
    CTTS_HIP_CHECK(hipMemset(*p, 0, bytes));
    return 0;
}
// ... and one released early leaves the record
static void dev_free(ctts_gpt* h, void* p) {
    if (!p) return;
    for (size_t i = 0; i < h->owned.size(); ++i) if (h->owned[i] == p) { h->owned.erase(h->owned.begin() + i); break; }
    (void)hipFree(p);
}

extern "C" int ctts_gpt_create(const ctts_gpt_cfg* c, ctts_gpt** out) {
    if (!c || !out) { ctts_set_error("null argument"); return 1; }
    if (c->hidden != 768 || c->inter != 3072 || c->heads * CTTS_HEAD_DIM != c->hidden) {
        ctts_set_error("this build is specialised to hidden=768, inter=3072, head_dim=64 (got %d/%d/%d heads)", c->hidden, c->inter, c->heads);
        return 1;
    }
    if (c->num_vq != CTTS_NUM_VQ || c->vocab_code > 640 || c->max_batch < 1 || c->max_batch > CTTS_MAX_B || c->max_seq < 2 ||
        (c->dtype != CTTS_DTYPE_F32 && c->dtype != CTTS_DTYPE_F16)) {
        ctts_set_error("unsupported configuration (num_vq=%d vocab=%d max_batch=%d dtype=%d)", c->num_vq, c->vocab_code, c->max_batch, c->dtype);
        return 1;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { ctts_set_error("no HIP device visible"); return 1; }
    ctts_gpt* h = new ctts_gpt();
    h->cfg = *c;
    h->H = c->hidden; h->I = c->inter; h->NH = c->heads; h->L = c->layers; h->V = c->vocab_code; h->NVQ = c->num_vq;
    h->esz = (c->dtype == CTTS_DTYPE_F16) ? 2 : 4;
    h->score_text_chunk = c->max_batch < SCORE_ROWS ? c->max_batch : SCORE_ROWS;
    h->split_rows = 8;                                           // both dtypes (the comment at split_rows)
    // both dtypes since round 5 (fp16 engines: half weights + half K / V in the image, fp32 activations).  fp16: up to 5 rows -- ms/step launch chain / persistent launch on the
    // final round-5 kernel (four edge waves, joint row sums; profiles/r05_step_time_vs_batch_fp16.jsonl): batch 1 0.370 / 0.235, 2: 0.393 / 0.276, 3: 0.423 / 0.312, 4: 0.425 / 0.346,
    // 5: 0.431 / 0.389 (round 6 with the 16-byte act granules: 0.229 / 0.268 / - / 0.342 / 0.380; the first version, two edge waves, had lost at 4 rows: 0.427 / 0.442)
    // fp32: 8 since round 6 (6..8 rows: two attention items per workgroup; ms/step launch chain / persistent launch at mean context 310: 6 rows 0.586 / 0.484, 7: 0.605 / 0.522,
    // 8: 0.617 / 0.557; at context 560: 6 rows 0.690 / 0.660, 8: 0.704 / 0.721 -> persist_pair_keys).  fp16 stays at 5: its chain is faster there (6 rows 0.467 / 0.489, 8: 0.472 / 0.550)
    h->persist_rows = (c->dtype == CTTS_DTYPE_F16) ? PL_MAXR_ONE : PL_MAXR;      // (ms/step launch chain / persistent launch at 5 rows, fp32: 0.540 / 0.389; fp16 at 4 rows: 0.425 / 0.345)
    h->attn_wide_blocks = (c->dtype == CTTS_DTYPE_F16) ? 4096 : 512;
    h->nbg2_rows = (c->dtype == CTTS_DTYPE_F16) ? 57 : 81;
    h->down_sk_rows = 9;                                         // = the first batch size of the packed-residual path (split_rows + 1)
    // Diagnostic switches exist only in builds with -DCTTS_DIAG (python -m chatttsplus_amd.build --diag) and are read HERE, once: the
    // product library takes no behaviour from the environment on its launch paths (diag_env() is a constant null there).
    if (const char* sr = diag_env("CTTS_SPLIT_ROWS")) { h->split_rows = atoi(sr); if (h->split_rows > 32) h->split_rows = 32; }
    if (const char* nr = diag_env("CTTS_NBG2_ROWS")) h->nbg2_rows = atoi(nr);
    if (const char* xm = diag_env("CTTS_XH")) h->xh_mode = atoi(xm) ? 1 : 0;
    if (const char* gs = diag_env("CTTS_GRAPH_STEPS")) { h->graph_steps = atoi(gs); if (h->graph_steps < 1) h->graph_steps = 1; }
    if (const char* e = diag_env("CTTS_SPLITS")) { const int v = atoi(e); if (v >= 1 && v <= SMAX) h->force_splits = v; }
    if (diag_env("CTTS_NO_PREPACK")) h->no_prepack = 1;
    if (const char* e = diag_env("CTTS_PREFILL_GEMM")) { const int v = atoi(e); h->prefill_gemm_rows = v > 1 ? v : (v == 1 ? 1536 : 0); }
    if (diag_env("CTTS_NO_XH_HEADS")) h->xh_heads = 0;
    if (const char* e = diag_env("CTTS_PREFILL_SPLIT")) h->split_rows_min = atoi(e);
    if (gemm_configure()) { delete h; return 1; }
    if (hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) {
        ctts_set_error("stream/event creation failed"); delete h; return 1;
    }
    *out = h;
    return 0;
}

// Persistent launches need all 256 workgroups resident at once: two processes that both run them on ONE device can starve each other until the
// spin limit (the engine then reports an error).  One advisory file lock per device and process keeps the mode to the first process that asks for
// it on that device; later processes (the 2-rank-on-one-GPU test, a second service on a shared box) quietly stay on the launch path.
static bool persist_device_lock(int dev) {
    static std::mutex mu;
    static std::map<int, int> fds;
    std::lock_guard<std::mutex> lk(mu);
    auto it = fds.find(dev);
    if (it != fds.end()) return it->second >= 0;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof(bus), dev) != hipSuccess) snprintf(bus, sizeof(bus), "dev%d", dev);
    for (char* c = bus; *c; ++c) if (*c == ':' || *c == '.' || *c == '/') *c = '_';
    char path[160];
    snprintf(path, sizeof(path), "/tmp/ctts_persist_%s.lock", bus);
    int fd = open(path, O_CREAT | O_RDWR | O_CLOEXEC | O_NOFOLLOW, 0666);      // (never follows a planted symlink; not inherited by child processes)
    if (fd >= 0) (void)fchmod(fd, 0666);             // (the umask must not make the file another user's obstacle)
    else fd = open(path, O_RDONLY | O_CLOEXEC | O_NOFOLLOW);      // a file left by another user: flock works on a read-only descriptor too
    if (fd >= 0 && flock(fd, LOCK_EX | LOCK_NB) != 0) { close(fd); fd = -1; }
    fds[dev] = fd;                                 // (kept for the life of the process)
    return fd >= 0;
}

// The persistent decode layer's device state: weight images (repacked on the device from the MFMA tile images: no host copy of the weights is
// needed after finalize), granule buffers, launch counter, error word.  `required`: the caller asked for the mode explicitly (an unmet precondition is
// an error); otherwise the mode is simply left off.
static int ensure_persist(ctts_gpt* h, bool required) {
    if (h->persist_ok || !h->finalized) return 0;               // (before finalize: checked by finalize)
    int dev = 0, cus = 0;
    CTTS_HIP_CHECK(hipGetDevice(&dev));
    CTTS_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const char* why = nullptr;
    if (h->L > 31) why = "at most 31 decoder layers";
    else if (cus < PL_BLOCKS) why = "the device has fewer than 256 compute units";
    else if (!persist_device_lock(dev)) why = "another process already runs persistent launches on this device";
    if (why) {
        h->persist_rows = 0;
        if (required) { ctts_set_error("persistent layers unavailable: %s", why); return 1; }
        return 0;
    }
    if (persist_configure()) return 1;
    if (dev_alloc(h, (void**)&h->pl_g, (size_t)PL_G_TOTAL * 8) || dev_alloc(h, (void**)&h->pl_epoch, 4)) return 1;
    if (!h->pl_error && dev_alloc(h, (void**)&h->pl_error, 4)) return 1;
    const unsigned one = 1;
    CTTS_HIP_CHECK(hipMemcpy(h->pl_epoch, &one, 4, hipMemcpyHostToDevice));
    h->persist_ok = true;
    return 0;
}
// the weight images, on first need (called outside stream capture: allocates, launches on the null stream, synchronises)
static int persist_images(ctts_gpt* h) {
    if (h->pimg != nullptr || !h->persist_ok) return 0;
    const size_t layer_bytes = PL_LAYER_BYTES / 4 * h->esz;
    // built into locals and published only when complete: a failed allocation or repack (an engine beside others on a full device) leaves the engine on the launch
    // chain -- the mode is an optimisation -- instead of failing the decode call that happened to need the images first, or leaving half-built ones behind
    char* img = nullptr; char* img_head = nullptr;
    bool ok = dev_alloc(h, (void**)&img, layer_bytes * h->L) == 0;
    for (int l = 0; ok && l < h->L; ++l)
        ok = launch_persist_repack(h->esz == 2, h->lw[l].qkv, h->lw[l].o, h->lw[l].gu, h->lw[l].d, img + layer_bytes * l, nullptr) == 0;
    ok = ok && dev_alloc(h, (void**)&img_head, (size_t)PL_GEMV_BLOCKS * PL_HEAD_FRAGS * 4 * h->esz) == 0;
    ok = ok && launch_persist_repack_heads(h->esz == 2, h->whead, (h->NVQ * h->V + 15) / 16, img_head, nullptr) == 0;
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        dev_free(h, img); dev_free(h, img_head);
        h->persist_rows = 0;                                     // (ctts_gpt_get_option reports it; "persistent_rows" can be set again)
        return 0;
    }
    h->pimg = img; h->pimg_head = img_head;
    return 0;
}

// Named engine options: explicit calls of the host side (hip_models.GPT(options=...)), never the environment.  One row per option: its field, how a value is clamped
// (v < lo -> below, v > hi -> above; OPT_FLAG: v != 0), whether it can be set / read, and what ctts_gpt_get_option reports while "batch_invariant" pins it (OPT_PIN: the
// stored value is kept for when the option is switched off; what the launches use meanwhile is stated at tuning()).  Options that do more than store an integer name a hook.
enum { OPT_W = 1, OPT_R = 2, OPT_RW = 3, OPT_FLAG = 4, OPT_PIN = 8 };
enum OptHook { HOOK_NONE, HOOK_BATCH_INV, HOOK_PREFILL_SPLIT, HOOK_SPLIT_DECODE, HOOK_PERSIST_ROWS, HOOK_TIMESTAMPS, HOOK_DECODE_SPLITS, HOOK_POLL };
struct OptRow { const char* name; int ctts_gpt::*field; int lo, below, hi, above; int flags; int pin; OptHook hook; };
#define OPT_MAX 0x7FFFFFFF
#define OPT_MIN(lo) lo, lo, OPT_MAX, OPT_MAX             // below lo -> lo
#define OPT_RANGE(lo, hi) lo, lo, hi, hi                 // clamped to lo..hi
#define OPT_ANY 0, 0, 0, 0                               // OPT_FLAG rows and hooks that do not clamp
static const OptRow g_options[] = {
    {"batch_invariant", &ctts_gpt::batch_inv, OPT_ANY, OPT_RW | OPT_FLAG, 0, HOOK_BATCH_INV},      // fp32 engines: bit-identical rows whatever the batch / schedule (see batch_inv); before or after finalize
    {"schedule_invariant", &ctts_gpt::batch_inv, OPT_ANY, OPT_RW | OPT_FLAG, 0, HOOK_BATCH_INV},   // the same field under its dtype-independent name: a synonym on fp32 engines, the only accepted setter on fp16 engines
    // prompt passes of >= this many rows use the head / tail fp16 split GEMMs (fp32 engines); 0 = never.  Before finalize: also decides whether the images are built; afterwards the
    // pass can be switched off (0: a checkpoint that leaves the fp16 range, see ctts_gpt_saturations) or moved while the images exist
    {"prefill_split_rows", &ctts_gpt::split_rows_min, OPT_MIN(0), OPT_RW | OPT_PIN, 1, HOOK_PREFILL_SPLIT},
    // fp32 engines: decode batches of >= this many rows multiply on the fp16 pipes with head / tail operands (0 = never; see split_dec_rows).  Before finalize: also decides whether the images are built
    {"split_decode_rows", &ctts_gpt::split_dec_rows, OPT_MIN(0), OPT_RW | OPT_PIN, 1, HOOK_SPLIT_DECODE},
    {"split_nbg2_rows", &ctts_gpt::split_nbg2_rows, OPT_MIN(17), OPT_RW | OPT_PIN, 0, HOOK_NONE},
    {"weight_prefetch_kb", &ctts_gpt::prefetch_kb, OPT_RANGE(0, 4096), OPT_RW, 0, HOOK_NONE},      // launch chain: KiB of the next launch's weights per prefetch workgroup (0 = no prefetch workgroups; see prefetch_kb)
    {"valu_rows", &ctts_gpt::valu_rows, OPT_RANGE(0, 4), OPT_RW | OPT_PIN, 0, HOOK_NONE},          // fp32 engines: decode batches of <= this many rows run their projections on the VALU instead of exact-f32 MFMA (0..4)
    // decode batches of <= this many rows run each layer as ONE persistent launch (0 = off); reads the EFFECTIVE value (0 when the mode is unavailable)
    {"persistent_rows", &ctts_gpt::persist_rows, OPT_RANGE(0, CTTS_PERSIST_MAX_ROWS), OPT_RW | OPT_PIN, 0, HOOK_PERSIST_ROWS},
    {"persistent_delay_lora", &ctts_gpt::persist_delay_u, 0, -1, 256, 256, OPT_RW, 0, HOOK_NONE},
    {"prefill_small_blocks", &ctts_gpt::prefill_small_blocks, OPT_MIN(0), OPT_RW, 0, HOOK_NONE},
    {"prefill_ring4_blocks", &ctts_gpt::prefill_ring4_blocks, OPT_MIN(0), OPT_RW, 0, HOOK_NONE},
    {"prefill_splitk_rows", &ctts_gpt::prefill_sk_rows, OPT_MIN(0), OPT_RW | OPT_PIN, 0, HOOK_NONE},
    {"prefill_pp_blocks", &ctts_gpt::prefill_pp_blocks, -4, 0, OPT_MAX, OPT_MAX, OPT_RW, 0, HOOK_NONE},      // -3 / -4: always the counter-phased kernel with that many n tiles per wave (tests, A/B)
    {"attn_wide_blocks", &ctts_gpt::attn_wide_blocks, OPT_MIN(0), OPT_RW | OPT_PIN, OPT_MAX, HOOK_NONE},
    {"persistent_share_keys", &ctts_gpt::persist_share_keys, 64, 384, OPT_MAX, OPT_MAX, OPT_RW, 0, HOOK_NONE},
    {"persistent_lora", &ctts_gpt::persist_lora, OPT_ANY, OPT_RW | OPT_FLAG, 0, HOOK_NONE},        // 1 (default): rows with per-utterance adapters stay on the persistent launch; 0 = they take the launch chain
    {"persistent_heads", &ctts_gpt::persist_heads, OPT_ANY, OPT_RW | OPT_FLAG, 0, HOOK_NONE},      // 1 (default): the persistent launch that ends the stack also runs the final norm + heads; 0 = the separate heads launch
    {"persistent_layers_per_launch", &ctts_gpt::persist_lpl, OPT_MIN(0), OPT_RW, 0, HOOK_NONE},    // 0 = the whole stack in one launch (default); 1 = one launch per layer
    {"persistent_schedule", &ctts_gpt::persist_sched, 1, 1, 3, 1, OPT_RW, 0, HOOK_NONE},           // 1 / 2: see persist_layer.hip
    {"lora_fold", &ctts_gpt::lora_fold, 0, 1, 3, 1, OPT_RW, 0, HOOK_NONE},                         // per-utterance adapters at decode: 1 = workers inside the QKV / o_proj launches, 0 = two more launches per layer
    {"persistent_fault", &ctts_gpt::persist_fault, OPT_MIN(0), OPT_RW, 0, HOOK_NONE},              // test hook: a withheld hand-off; every wait is bounded, ctts_gpt_progress reports the edge
    {"persistent_pair_keys", &ctts_gpt::persist_pair_keys, OPT_MIN(0), OPT_RW, 0, HOOK_NONE},
    {"persistent_max_keys", &ctts_gpt::persist_max_keys, OPT_MIN(0), OPT_RW, 0, HOOK_NONE},
    {"persistent_splits", &ctts_gpt::persist_splits, OPT_RANGE(0, PL_SMAX), OPT_RW, 0, HOOK_NONE},
    {"persistent_pace", &ctts_gpt::persist_pace, 0, -1, 64, 64, OPT_RW, 0, HOOK_NONE},             // SCHED 3: ~128-cycle units between two paced weight requests of a wave (< 0: by row count)
    {"persistent_delay_att", &ctts_gpt::persist_delay_att, OPT_RANGE(0, 256), OPT_RW, 0, HOOK_NONE},
    {"persistent_delay", &ctts_gpt::persist_delay, OPT_RANGE(0, 256), OPT_RW, 0, HOOK_NONE},
    {"persistent_delay_act", &ctts_gpt::persist_delay_act, OPT_RANGE(0, 256), OPT_RW, 0, HOOK_NONE},
    {"persistent_delay_x", &ctts_gpt::persist_delay_x, OPT_RANGE(0, 256), OPT_RW, 0, HOOK_NONE},
    {"persistent_nap_qkv", &ctts_gpt::persist_nap_qkv, OPT_RANGE(0, 256), OPT_RW, 0, HOOK_NONE},
    {"persistent_nap", &ctts_gpt::persist_nap, OPT_RANGE(0, 256), OPT_RW, 0, HOOK_NONE},
    {"persistent_poll", &ctts_gpt::persist_poll, OPT_ANY, OPT_RW, 0, HOOK_POLL},                   // bit 0: sentinel granules before the full sweeps (< 0: by row count)
    {"persistent_timestamps", &ctts_gpt::pl_ts_on, OPT_ANY, OPT_RW | OPT_FLAG, 0, HOOK_TIMESTAMPS},      // diagnostics: every workgroup of a persistent launch records wall_clock64 marks (ctts_gpt_debug_read "pl_ts")
    {"decode_splits", &ctts_gpt::force_splits, OPT_ANY, OPT_RW | OPT_PIN, 1, HOOK_DECODE_SPLITS},  // key splits of the decode attention (0 = the decode_splits policy); out-of-range values are refused
    {"split_rows", &ctts_gpt::split_rows, OPT_RANGE(0, 32), OPT_RW | OPT_PIN, 0, HOOK_NONE},       // decode batches up to this size run the down projection as split-K launch slices
    {"nbg2_rows", &ctts_gpt::nbg2_rows, OPT_MIN(17), OPT_RW | OPT_PIN, 0, HOOK_NONE},              // decode batches of >= this many rows use 32-row blocks (see nbg2_rows)
    {"down_splitk_rows", &ctts_gpt::down_sk_rows, OPT_MIN(0), OPT_RW | OPT_PIN, 1, HOOK_NONE},     // see down_sk_rows
    {"graph_steps", &ctts_gpt::graph_steps, OPT_RANGE(1, 64), OPT_RW, 0, HOOK_NONE},
    {"graph_steps_persistent", &ctts_gpt::graph_steps_persist, OPT_RANGE(1, 64), OPT_RW, 0, HOOK_NONE},
    {"text_rows_live", &ctts_gpt::text_live, OPT_ANY, OPT_R, 0, HOOK_NONE},    // read only: rows of the decode batch whose mode is 1 (ctts_gpt_enable_text_rows); > 0 = every step runs the text head and the text sampler too
    {"score_text_chunk", &ctts_gpt::score_text_chunk, OPT_ANY, OPT_R, 0, HOOK_NONE},      // read only: rows per text-head launch of ctts_gpt_score_text (= max_batch: the decode step's launch shape)
    {"lora_mlp_live", &ctts_gpt::lora_mlp, OPT_ANY, OPT_R, 0, HOOK_NONE},      // read only: 1 while a live row's adapter names gate / up / down (the two MLP launches per layer run, decode on the launch chain)
};
// the name under which this engine's dtype takes the contract (error messages)
static inline const char* inv_name(const ctts_gpt* h) { return h->cfg.dtype == CTTS_DTYPE_F16 ? "schedule_invariant" : "batch_invariant"; }
static const OptRow* find_option(const char* name, int access) {
    for (const OptRow& o : g_options) if (!strcmp(name, o.name)) return (o.flags & access) ? &o : nullptr;
    return nullptr;
}

extern "C" int ctts_gpt_get_option(ctts_gpt* h, const char* name, int* value) {
    if (!h || !name || !value) { ctts_set_error("get_option: null argument"); return 1; }
    const OptRow* o = find_option(name, OPT_R);
    if (!o) { ctts_set_error("get_option: unknown option '%s'", name); return 1; }
    if (h->batch_inv && (o->flags & OPT_PIN))          // what the launches use while the option is on (the tuning values set meanwhile are kept for when it is switched off)
        *value = (h->cfg.dtype == CTTS_DTYPE_F16 && (o->hook == HOOK_PREFILL_SPLIT || o->hook == HOOK_SPLIT_DECODE)) ? 0 : o->pin;      // (fp16 engines hold no head / tail images: both mechanisms read "never")
    else if (o->hook == HOOK_PERSIST_ROWS) *value = (h->persist_ok || !h->finalized) ? h->persist_rows : 0;
    else *value = h->*o->field;
    return 0;
}

// Options that shape the launches bump `opt_gen`, which is part of the decode-graph key, so graphs captured under other settings are not replayed.
extern "C" int ctts_gpt_set_option(ctts_gpt* h, const char* name, int value) {
    if (!h || !name) { ctts_set_error("set_option: null argument"); return 1; }
    const OptRow* o = find_option(name, OPT_W);
    if (!o) { ctts_set_error("set_option: unknown option '%s'", name); return 1; }
    const bool images = h->split_ok && h->wsplit;      // (refusals first: a refused value changes nothing)
    if (o->hook == HOOK_BATCH_INV) {
        // fp16 engines take the contract under its dtype-independent name only (their pinned stack needs no head / tail images)
        if (h->cfg.dtype != CTTS_DTYPE_F32 && strcmp(name, "schedule_invariant")) { ctts_set_error("set_option(batch_invariant): fp32 (parity) engines only; an fp16 engine takes the contract as \"schedule_invariant\""); return 1; }
        if (value && h->cfg.dtype == CTTS_DTYPE_F32 && h->finalized && !(images && h->whead_sp)) {
            ctts_set_error("set_option(%s): this engine holds no head / tail weight images (a weight beyond the fp16 range, or split_decode_rows and prefill_split_rows were 0 at finalize)", name);
            return 1;
        }
    } else if (o->hook == HOOK_PREFILL_SPLIT || o->hook == HOOK_SPLIT_DECODE) {
        if (h->finalized && value > 0 && !images) { ctts_set_error("set_option(%s): this engine holds no head / tail weight images (fp16 engine, a weight beyond the fp16 range, or the option was 0 at finalize)", name); return 1; }
    } else if (o->hook == HOOK_DECODE_SPLITS) {
        if (value < 0 || value > SMAX) { ctts_set_error("set_option(decode_splits): 0..%d", SMAX); return 1; }
    } else if (o->hook == HOOK_TIMESTAMPS && value && !h->pl_ts && dev_alloc(h, (void**)&h->pl_ts, (size_t)PL_BLOCKS * 10 * 8)) return 1;
    if (o->flags & OPT_FLAG) value = value ? 1 : 0;
    else if (o->hook == HOOK_POLL) value = value < 0 ? -1 : (value & 1);
    else if (o->hook != HOOK_DECODE_SPLITS) value = value < o->lo ? o->below : (value > o->hi ? o->above : value);
    h->*o->field = value;
    if (o->hook == HOOK_PERSIST_ROWS && value > 0 && ensure_persist(h, true)) { h->persist_rows = 0; return 1; }
    h->opt_gen++;
    return 0;
}

extern "C" void ctts_gpt_destroy(ctts_gpt* h) {
    if (!h) return;
    for (auto& kv : h->graphs) { (void)hipGraphExecDestroy(kv.second.exec); (void)hipGraphDestroy(kv.second.graph); }
    for (void* b : h->owned) (void)hipFree(b);
    if (h->host_pin) (void)hipHostFree(h->host_pin);
    if (h->guide_pin) (void)hipHostFree(h->guide_pin);
    for (hipEvent_t e : h->guide_ev) if (e) (void)hipEventDestroy(e);
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
}

// The 196 keys of the reference's GPT state dict: 9 per decoder layer, gpt.norm, 4 emb_code, emb_text, 2 + 8 weight-norm
// parametrizations of the heads.
static bool known_weight_key(const ctts_gpt* h, const std::string& n) {
    int l = -1, consumed = 0;
    if (sscanf(n.c_str(), "gpt.layers.%d.%n", &l, &consumed) == 1 && consumed > 0) {
        if (l < 0 || l >= h->L) return false;
        const std::string rest = n.substr(consumed);
        static const char* per_layer[] = {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
                                          "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight", "input_layernorm.weight",
                                          "post_attention_layernorm.weight"};
        for (const char* k : per_layer) if (rest == k) return true;
        return false;
    }
    if (n == "gpt.norm.weight" || n == "emb_text.weight" || n == "head_text.parametrizations.weight.original0" ||
        n == "head_text.parametrizations.weight.original1") return true;
    int i = -1; consumed = 0;
    if (sscanf(n.c_str(), "emb_code.%d.weigh%n", &i, &consumed) == 1 && consumed > 0) return i >= 0 && i < h->NVQ && n.substr(consumed) == "t";
    if (sscanf(n.c_str(), "head_code.%d.parametrizations.weight.origina%n", &i, &consumed) == 1 && consumed > 0) {
        const std::string rest = n.substr(consumed);
        return i >= 0 && i < h->NVQ && (rest == "l0" || rest == "l1");
    }
    return false;
}

extern "C" int ctts_gpt_set_weight(ctts_gpt* h, const char* name, const float* data, size_t numel) {
    if (!h || !name || !data) { ctts_set_error("null argument"); return 1; }
    if (h->finalized) { ctts_set_error("weights already finalized"); return 1; }
    std::string n(name);
    if (!known_weight_key(h, n)) {          // strict load, like the reference's load_state_dict(strict=True) (gpt.py:84-85)
        ctts_set_error("set_weight: unexpected key '%s' (not a tensor of the ChatTTS GPT state dict)", name);
        return 1;
    }
    h->host[n].assign(data, data + numel);
    return 0;
}

static int lora_target_index(const char* t);
static inline int lora_target_out(const ctts_gpt* h, int t) { return (t == 4 || t == 5) ? h->I : h->H; }      // (out, in) of target t: gate / up I x H, down H x I, q/k/v/o H x H
static inline int lora_target_in(const ctts_gpt* h, int t) { return t == 6 ? h->I : h->H; }
extern "C" int ctts_gpt_merge_lora(ctts_gpt* h, int layer, const char* target, const float* A, const float* B, int r, float scale) {
    if (!h || h->finalized) { ctts_set_error("merge_lora must precede finalize"); return 1; }
    if (!target || !A || !B || r < 1) { ctts_set_error("merge_lora: null argument or r %d < 1", r); return 1; }
    const int t = lora_target_index(target);
    if (t < 0) { ctts_set_error("merge_lora: unknown target '%s' (q_proj k_proj v_proj o_proj gate_proj up_proj down_proj)", target); return 1; }
    char key[128];
    snprintf(key, sizeof(key), "gpt.layers.%d.%s.%s.weight", layer, t < 4 ? "self_attn" : "mlp", target);
    auto it = h->host.find(key);
    if (it == h->host.end()) { ctts_set_error("merge_lora: %s not loaded", key); return 1; }
    const int out = lora_target_out(h, t), in = lora_target_in(h, t);      // A [r][in], B [out][r] (llama.py:214,737-739: gate / up 3072 x 768, down 768 x 3072)
    if (it->second.size() != (size_t)out * in) { ctts_set_error("merge_lora: %s holds %zu values, not %d x %d", key, it->second.size(), out, in); return 1; }
    std::vector<float>& W = it->second;
    // peft merge_and_unload: W' = W + scale * B @ A   (pipeline:420-432; scale = lora_alpha / r)
    for (int o = 0; o < out; ++o)
        for (int i = 0; i < in; ++i) {
            float acc = 0.f;
            for (int k = 0; k < r; ++k) acc += B[(size_t)o * r + k] * A[(size_t)k * in + i];
            W[(size_t)o * in + i] += scale * acc;
        }
    return 0;
}

// ---- per-utterance LoRA (lora.hip) ---------------------------------------------------------------
static int lora_target_index(const char* t) {
    static const char* names[7] = {"q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"};
    for (int i = 0; i < 7; ++i) if (t && !strcmp(t, names[i])) return i;
    return -1;
}
static int lora_ensure_storage(ctts_gpt* h) {
    if (h->lora_A) return 0;
    const size_t per = (size_t)h->L * CTTS_MAX_ADAPTERS * 4 * 16 * h->H;
    if (dev_alloc(h, (void**)&h->lora_Af, per / 4 * 3 * 4)) return 1;
    CTTS_HIP_CHECK(hipMemset(h->lora_Af, 0, per / 4 * 3 * 4));
    if (dev_alloc(h, (void**)&h->lora_A, per * 4) || dev_alloc(h, (void**)&h->lora_B, per * 4) ||
        dev_alloc(h, (void**)&h->lora_scale, (size_t)h->L * CTTS_MAX_ADAPTERS * 4 * 4) || dev_alloc(h, (void**)&h->lora_slot_of_seq, CTTS_MAX_B * 4) ||
        dev_alloc(h, (void**)&h->lora_dqkv, (size_t)h->pass_rows * 3 * h->H * 4) || dev_alloc(h, (void**)&h->lora_do, (size_t)h->pass_rows * h->H * 4))
        return 1;
    CTTS_HIP_CHECK(hipMemset(h->lora_slot_of_seq, 0xFF, CTTS_MAX_B * 4));
    if (dev_alloc(h, (void**)&h->lora_g, (size_t)CTTS_MAX_B * 4 * h->H * 8)) return 1;           // [rows][3][768] q/k/v | [rows][768] o_proj
    CTTS_HIP_CHECK(hipMemset(h->lora_g, 0, (size_t)CTTS_MAX_B * 4 * h->H * 8));                 // tag 0 never matches (tags start at 64)
    if (!h->pl_error) { if (dev_alloc(h, (void**)&h->pl_error, 4)) return 1; CTTS_HIP_CHECK(hipMemset(h->pl_error, 0, 4)); }
    return 0;
}
static int lora_ensure_mlp_storage(ctts_gpt* h) {
    if (!h->lora_mrank.empty()) return 0;           // (set last: a failed allocation leaves it empty, and the next call takes up where this one stopped)
    const size_t slots = (size_t)h->L * CTTS_MAX_ADAPTERS, H = h->H, I = h->I;
    struct { float** p; size_t n; } tabs[] = {{&h->lora_mA_gu, slots * 2 * 16 * H}, {&h->lora_mB_gu, slots * 2 * 16 * I}, {&h->lora_mA_d, slots * 16 * I},
                                              {&h->lora_mB_d, slots * 16 * H}, {&h->lora_mscale, slots * 4}};
    for (auto& t : tabs) {
        if (*t.p == nullptr && dev_alloc(h, (void**)t.p, t.n * 4)) return 1;
        CTTS_HIP_CHECK(hipMemset(*t.p, 0, t.n * 4));
    }
    if (h->ln2_host.size() != (size_t)h->L * H) { ctts_set_error("set_adapter: the post-attention RMSNorm weights were not kept at finalize"); return 1; }
    if (h->ln2 == nullptr && dev_alloc(h, (void**)&h->ln2, h->ln2_host.size() * 4)) return 1;
    CTTS_HIP_CHECK(hipMemcpy(h->ln2, h->ln2_host.data(), h->ln2_host.size() * 4, hipMemcpyHostToDevice));
    h->lora_mrank.assign(slots * 3, 0);
    return 0;
}
// The rows' gate / up terms [rows of a pass][gate | up][3072] fp32 -- 24 KB per prompt row, 402 MB on an engine sized for 16384-row passes: allocated when a LIVE row first
// selects a slot that holds an MLP target (an MLP adapter that is resident but unused costs its tables only).  Called wherever lora_mlp can rise, outside graph capture.
static int lora_ensure_mlp_terms(ctts_gpt* h) {
    if (!h->lora_mlp || h->lora_dgu) return 0;
    return dev_alloc(h, (void**)&h->lora_dgu, (size_t)h->pass_rows * 2 * h->I * 4);
}
// does `slot` hold an MLP target in any layer?
static bool lora_slot_has_mlp(const ctts_gpt* h, int slot) {
    if (slot < 0 || h->lora_mrank.empty()) return false;
    for (int l = 0; l < h->L; ++l)
        for (int t = 0; t < 3; ++t) if (h->lora_mrank[((size_t)l * CTTS_MAX_ADAPTERS + slot) * 3 + t]) return true;
    return false;
}
// lora_rows / lora_mlp of n adapter slots; allocates the MLP terms where lora_mlp rises
template <class SlotOf>
static int lora_summary(ctts_gpt* h, int n, SlotOf slot_of) {
    h->lora_rows = 0; h->lora_mlp = 0;
    for (int i = 0; i < n; ++i) { h->lora_rows |= slot_of(i) >= 0; h->lora_mlp |= lora_slot_has_mlp(h, slot_of(i)); }
    return lora_ensure_mlp_terms(h);
}
// The summaries of `rows` (text_live, lora_rows, lora_mlp): called wherever the row set or a row's mode / slot changes -- begin, admit, grow, compact, admit_adapters,
// seat_row_adapters, set_row_adapters, the end of the state
static int refresh_rows(ctts_gpt* h) {
    h->text_live = 0;
    for (const HostRow& r : h->rows) h->text_live += r.mode;
    return lora_summary(h, (int)h->rows.size(), [h](int r) { return h->rows[r].slot; });
}
// The rows' adapter slots as the decode launches and the graph key carry them: one byte per row, -1 (0xFF) past the batch
static void row_slot_bytes(const ctts_gpt* h, signed char* out, int n) {
    for (int r = 0; r < n; ++r) out[r] = r < (int)h->rows.size() ? (signed char)h->rows[r].slot : (signed char)-1;
}
// gate_proj / up_proj / down_proj (t = 4 / 5 / 6) of one layer into the slot's MLP tables
static int lora_set_mlp_target(ctts_gpt* h, int slot, int layer, int t, const float* A, const float* B, int r, float scale) {
    if (h->H != 768 || h->I != 3072) { ctts_set_error("set_adapter: MLP targets need hidden 768 / intermediate 3072 (engine: %d / %d)", h->H, h->I); return 1; }
    if (lora_ensure_storage(h) || lora_ensure_mlp_storage(h)) return 1;
    const int out = lora_target_out(h, t), in = lora_target_in(h, t), m = t - 4;
    std::vector<float> a16((size_t)16 * in, 0.f), b16((size_t)16 * out, 0.f);
    memcpy(a16.data(), A, (size_t)r * in * 4);
    for (int n = 0; n < out; ++n) for (int k = 0; k < r; ++k) b16[(size_t)k * out + n] = B[(size_t)n * r + k];       // rank-major like A
    const size_t ls = (size_t)layer * CTTS_MAX_ADAPTERS + slot;
    float* dA = m < 2 ? h->lora_mA_gu + (ls * 2 + m) * 16 * in : h->lora_mA_d + ls * 16 * in;
    float* dB = m < 2 ? h->lora_mB_gu + (ls * 2 + m) * 16 * out : h->lora_mB_d + ls * 16 * out;
    CTTS_HIP_CHECK(hipMemcpy(dA, a16.data(), a16.size() * 4, hipMemcpyHostToDevice));
    CTTS_HIP_CHECK(hipMemcpy(dB, b16.data(), b16.size() * 4, hipMemcpyHostToDevice));
    CTTS_HIP_CHECK(hipMemcpy(h->lora_mscale + ls * 4 + m, &scale, 4, hipMemcpyHostToDevice));
    h->lora_mrank[ls * 3 + m] = (signed char)r;
    h->opt_gen++;                                   // which launches a step takes depends on the slots' targets: captured graphs are stale
    return 0;
}
extern "C" int ctts_gpt_set_adapter(ctts_gpt* h, int slot, int layer, const char* target, const float* A, const float* B, int r, float scale) {
    if (!h || !h->finalized || !A || !B) { ctts_set_error("set_adapter: handle not finalized or null argument"); return 1; }
    const int t = lora_target_index(target);
    if (slot < 0 || slot >= CTTS_MAX_ADAPTERS || layer < 0 || layer >= h->L || t < 0 || r < 1 || r > 16) {
        ctts_set_error("set_adapter: slot %d / layer %d / target %s / r %d out of range", slot, layer, target ? target : "(null)", r);
        return 1;
    }
    if (t >= 4) return lora_set_mlp_target(h, slot, layer, t, A, B, r, scale);
    if (lora_ensure_storage(h)) return 1;
    const int H = h->H;
    std::vector<float> a16((size_t)16 * H, 0.f), b16((size_t)H * 16, 0.f);
    for (int k = 0; k < r; ++k) memcpy(&a16[(size_t)k * H], A + (size_t)k * H, (size_t)H * 4);
    for (int n = 0; n < H; ++n) for (int k = 0; k < r; ++k) b16[(size_t)k * H + n] = B[(size_t)n * r + k];       // rank-major like A: rank r reads r rows
    const size_t off = (((size_t)layer * CTTS_MAX_ADAPTERS + slot) * 4 + t) * 16 * H;
    if (t < 3) {                                    // the persistent launch's copy: columns times the layer's input RMSNorm weight (its waves see x * rs, not w * (x * rs))
        if (h->ln1_host.empty()) { h->ln1_host.resize((size_t)h->L * H); CTTS_HIP_CHECK(hipMemcpy(h->ln1_host.data(), h->ln1, h->ln1_host.size() * 4, hipMemcpyDeviceToHost)); }
        std::vector<float> af(a16);
        const float* w = &h->ln1_host[(size_t)layer * H];
        for (int k = 0; k < r; ++k) for (int c = 0; c < H; ++c) af[(size_t)k * H + c] *= w[c];
        CTTS_HIP_CHECK(hipMemcpy(h->lora_Af + (((size_t)layer * CTTS_MAX_ADAPTERS + slot) * 3 + t) * 16 * H, af.data(), af.size() * 4, hipMemcpyHostToDevice));
    }
    CTTS_HIP_CHECK(hipMemcpy(h->lora_A + off, a16.data(), a16.size() * 4, hipMemcpyHostToDevice));
    CTTS_HIP_CHECK(hipMemcpy(h->lora_B + off, b16.data(), b16.size() * 4, hipMemcpyHostToDevice));
    CTTS_HIP_CHECK(hipMemcpy(h->lora_scale + ((size_t)layer * CTTS_MAX_ADAPTERS + slot) * 4 + t, &scale, 4, hipMemcpyHostToDevice));
    if (h->lora_rank.empty()) h->lora_rank.assign((size_t)h->L * CTTS_MAX_ADAPTERS * 4, 0);
    h->lora_rank[((size_t)layer * CTTS_MAX_ADAPTERS + slot) * 4 + t] = (signed char)r;
    h->opt_gen++;                                   // the ranks are kernel arguments of the folded launches: captured graphs are stale
    return 0;
}
extern "C" int ctts_gpt_clear_adapter(ctts_gpt* h, int slot) {
    if (!h || slot < 0 || slot >= CTTS_MAX_ADAPTERS) { ctts_set_error("clear_adapter: bad slot"); return 1; }
    if (!h->lora_A) return 0;
    const size_t per = (size_t)4 * 16 * h->H;
    for (int l = 0; l < h->L; ++l) {
        const size_t off = ((size_t)l * CTTS_MAX_ADAPTERS + slot) * per;
        CTTS_HIP_CHECK(hipMemset(h->lora_Af + off / 4 * 3, 0, per / 4 * 3 * 4));
        CTTS_HIP_CHECK(hipMemset(h->lora_A + off, 0, per * 4));
        CTTS_HIP_CHECK(hipMemset(h->lora_B + off, 0, per * 4));
        CTTS_HIP_CHECK(hipMemset(h->lora_scale + ((size_t)l * CTTS_MAX_ADAPTERS + slot) * 4, 0, 16));
        if (!h->lora_rank.empty()) for (int t = 0; t < 4; ++t) h->lora_rank[((size_t)l * CTTS_MAX_ADAPTERS + slot) * 4 + t] = 0;
        if (h->lora_mA_gu) {
            const size_t ls = (size_t)l * CTTS_MAX_ADAPTERS + slot, H = h->H, I = h->I;
            CTTS_HIP_CHECK(hipMemset(h->lora_mA_gu + ls * 2 * 16 * H, 0, 2 * 16 * H * 4));
            CTTS_HIP_CHECK(hipMemset(h->lora_mB_gu + ls * 2 * 16 * I, 0, 2 * 16 * I * 4));
            CTTS_HIP_CHECK(hipMemset(h->lora_mA_d + ls * 16 * I, 0, 16 * I * 4));
            CTTS_HIP_CHECK(hipMemset(h->lora_mB_d + ls * 16 * H, 0, 16 * H * 4));
            CTTS_HIP_CHECK(hipMemset(h->lora_mscale + ls * 4, 0, 16));
            for (int t = 0; t < 3; ++t) h->lora_mrank[ls * 3 + t] = 0;
        }
    }
    h->opt_gen++;
    return 0;
}
extern "C" int ctts_gpt_set_row_adapters(ctts_gpt* h, const int32_t* slots, int B) {
    if (!h || !h->finalized) { ctts_set_error("set_row_adapters: handle not finalized"); return 1; }
    auto clear_rows = [h]() -> int {              // no row carries an adapter: also forget what an earlier request's rows carried (ctts_gpt_admit_adapters builds on these)
        h->req.slots.clear();
        if (!h->lora_slot_host.empty()) h->lora_slot_host.assign(CTTS_MAX_B, -1);
        for (HostRow& r : h->rows) r.slot = -1;
        if (h->lora_slot_of_seq) CTTS_HIP_CHECK(hipMemset(h->lora_slot_of_seq, 0xFF, CTTS_MAX_B * 4));
        return refresh_rows(h);
    };
    if (!slots || B <= 0) return clear_rows();
    if (B > CTTS_MAX_B) { ctts_set_error("set_row_adapters: B=%d > %d", B, CTTS_MAX_B); return 1; }
    bool any = false;
    for (int b = 0; b < B; ++b) {
        if (slots[b] >= CTTS_MAX_ADAPTERS) { ctts_set_error("set_row_adapters: slot %d out of range", slots[b]); return 1; }
        any = any || slots[b] >= 0;
    }
    if (!any) return clear_rows();
    if (lora_ensure_storage(h)) return 1;
    std::vector<int> tab(CTTS_MAX_B, -1);
    for (int b = 0; b < B; ++b) tab[b] = slots[b] < 0 ? -1 : slots[b];
    CTTS_HIP_CHECK(hipMemcpy(h->lora_slot_of_seq, tab.data(), CTTS_MAX_B * 4, hipMemcpyHostToDevice));
    h->lora_slot_host = h->req.slots = tab;
    for (HostRow& r : h->rows) r.slot = tab[r.seq];      // (a row's slot is its lane's, always: compaction moves the row, the lane table stays)
    return lora_summary(h, B, [&tab](int b) { return tab[b]; });      // the sequences of the request: the next begin seats them (seat_row_adapters)
}

// ---- per-utterance sampling knobs (RowSampling, common.h) ----------------------------------------
static_assert(sizeof(ctts_row_sampling) == sizeof(RowSampling), "ctts_row_sampling and RowSampling share one layout");
// ctts_sampler_cfg -> the device copy the kernels read (ctts_gpt_begin, stand-alone sampler)
static SamplerCfgDev cfg_of_abi(const ctts_sampler_cfg& sc) {
    SamplerCfgDev c = {};
    memcpy(c.temperature, sc.temperature, sizeof(sc.temperature));
    c.top_p_threshold = sc.top_p_threshold; c.top_k = sc.top_k; c.min_keep = sc.min_tokens_to_keep;
    c.use_penalty = sc.use_penalty; memcpy(c.penalty_table, sc.penalty_table, sizeof(sc.penalty_table));
    c.past_window = sc.past_window; c.max_input_ids = sc.max_input_ids; c.eos = sc.eos_token;
    c.min_new = sc.min_new_token; c.max_new = sc.max_new_token;
    return c;
}
static RowSampling knobs_of_cfg(const SamplerCfgDev& c) {
    RowSampling r = {};
    memcpy(r.temperature, c.temperature, sizeof(r.temperature));
    r.top_p_threshold = c.top_p_threshold; r.top_k = c.top_k; r.min_keep = c.min_keep; r.use_penalty = c.use_penalty;
    memcpy(r.penalty_table, c.penalty_table, sizeof(r.penalty_table));
    r.past_window = c.past_window; r.min_new = c.min_new;
    return r;
}
static RowSampling knobs_of_abi(const ctts_row_sampling& p) {
    RowSampling r;
    memcpy(&r, &p, sizeof(r));
    r.pad = 0;
    return r;
}
// field by field (not the bytes: nothing may hang on two builders' padding)
static bool same_knobs(const RowSampling& a, const RowSampling& b) {
    for (int v = 0; v < CTTS_NUM_VQ; ++v) if (a.temperature[v] != b.temperature[v]) return false;
    for (int i = 0; i < 17; ++i) if (a.penalty_table[i] != b.penalty_table[i]) return false;
    return a.top_p_threshold == b.top_p_threshold && a.top_k == b.top_k && a.min_keep == b.min_keep && a.use_penalty == b.use_penalty &&
           a.past_window == b.past_window && a.min_new == b.min_new;
}
static int check_knobs(const ctts_row_sampling& p, int max_new, const char* who, int i) {
    for (int v = 0; v < CTTS_NUM_VQ; ++v)
        if (!std::isfinite(p.temperature[v]) || !(p.temperature[v] > 0.f)) { ctts_set_error("%s: entry %d: temperature[%d] = %g (must be finite and > 0)", who, i, v, (double)p.temperature[v]); return 1; }
    if (p.top_k < 0) { ctts_set_error("%s: entry %d: top_k = %d < 0", who, i, p.top_k); return 1; }
    if (p.min_tokens_to_keep < 1) { ctts_set_error("%s: entry %d: min_tokens_to_keep = %d < 1", who, i, p.min_tokens_to_keep); return 1; }
    if (p.past_window < 1 || p.past_window > 16) { ctts_set_error("%s: entry %d: past_window = %d outside 1..16 (the penalty ring is 16 deep)", who, i, p.past_window); return 1; }
    if (p.min_new_token > max_new) { ctts_set_error("%s: entry %d: min_new_token = %d > max_new_token = %d", who, i, p.min_new_token, max_new); return 1; }
    return 0;
}
extern "C" int ctts_gpt_set_row_sampling(ctts_gpt* h, const ctts_row_sampling* per_seq, int B) {
    if (!h) { ctts_set_error("set_row_sampling: null handle"); return 1; }
    if (!per_seq || B <= 0) { h->req.knobs.clear(); return 0; }
    if (B > CTTS_MAX_B) { ctts_set_error("set_row_sampling: B=%d > %d", B, CTTS_MAX_B); return 1; }
    h->req.knobs.assign(B, RowSampling{});
    for (int b = 0; b < B; ++b) h->req.knobs[b] = knobs_of_abi(per_seq[b]);      // checked by begin, against that call's max_new_token
    return 0;
}
// The `rows` argument of admit / cancel / admit_sampling / admit_modes / admit_adapters: every entry a row of the batch and, with `distinct`, none named twice; entry(i)
// checks what else the caller holds for entry i, right after its row (the first fault of the first faulty entry is the one reported)
static int rows_only(int) { return 0; }
template <class Entry = int (*)(int)>
static int check_rows(const ctts_gpt* h, const char* who, int n, const int32_t* rows, bool distinct, Entry entry = rows_only) {
    bool named[CTTS_MAX_B] = {};
    for (int i = 0; i < n; ++i) {
        if (rows[i] < 0 || rows[i] >= h->B) { ctts_set_error("%s: row %d of %d", who, rows[i], h->B); return 1; }
        if (distinct && named[rows[i]]) { ctts_set_error("%s: row %d named twice", who, rows[i]); return 1; }
        named[rows[i]] = true;
        if (entry(i)) return 1;
    }
    return 0;
}
// a NextCall list holds one entry per row: the last value named for it
template <typename V> static void name_row(std::vector<std::pair<int, V>>& list, int row, const V& v) {
    for (auto& e : list) if (e.first == row) { e.second = v; return; }
    list.emplace_back(row, v);
}
extern "C" int ctts_gpt_admit_sampling(ctts_gpt* h, int n, const int32_t* rows, const ctts_row_sampling* p, void* stream) {
    (void)stream;        // host-side request: the next ctts_gpt_admit uploads the entries
    if (!h || h->B == 0 || !rows || !p || n < 0) { ctts_set_error("admit_sampling: call begin first / null argument"); return 1; }
    if (h->text_mode) { ctts_set_error("admit_sampling: per-utterance sampling parameters are code mode only (the refine-text pass keeps the call's values)"); return 1; }
    if (check_rows(h, "admit_sampling", n, rows, false, [&](int i) { return check_knobs(p[i], h->sc.max_new, "admit_sampling", i); })) return 1;
    for (int i = 0; i < n; ++i) name_row(h->next.knobs, rows[i], knobs_of_abi(p[i]));
    return 0;
}

// ---- packing ---------------------------------------------------------------------------------
template <typename WT> static inline WT cvt(float v);
template <> inline float cvt<float>(float v) { return v; }
template <> inline half_t cvt<half_t>(float v) { return (half_t)v; }

// rows(pr) -> pointer to the source row (K floats) or nullptr for zero padding
template <typename WT, typename RowFn>
static void pack_tiles(WT* dst, int n_row_tiles, int K, RowFn rows, const float* colscale = nullptr) {
    constexpr int KT = WTraits<WT>::KT, EPL = WTraits<WT>::EPL;
    const int ktiles = K / KT;
    for (int rt = 0; rt < n_row_tiles; ++rt)
        for (int i = 0; i < 16; ++i) {
            const float* src = rows(rt * 16 + i);
            for (int kt = 0; kt < ktiles; ++kt)
                for (int kq = 0; kq < 4; ++kq) {
                    WT* d = dst + (((size_t)rt * ktiles + kt) * 64 + i + 16 * kq) * EPL;
                    const int k0 = kt * KT + kq * EPL;
                    for (int j = 0; j < EPL; ++j) d[j] = src ? cvt<WT>(colscale ? src[k0 + j] * colscale[k0 + j] : src[k0 + j]) : cvt<WT>(0.f);
                }
        }
}

// head / tail fp16 images of 64 * W in the fp16 tile layout (prefill_split.hip): hi = fp16(v), lo = fp16(v - hi)
// Returns false when a (norm-folded) weight times 64 leaves the fp16 range (|w| >= 1023.5): the images would hold inf; the caller then keeps the
// engine on the exact fp32 prompt kernels.
template <typename RowFn>
static bool pack_tiles_split(half_t* dst, int n_row_tiles, int K, RowFn rows, const float* colscale = nullptr) {
    constexpr int KT = 32, EPL = 8;
    const int ktiles = K / KT;
    bool in_range = true;
    for (int rt = 0; rt < n_row_tiles; ++rt)
        for (int i = 0; i < 16; ++i) {
            const float* src = rows(rt * 16 + i);
            for (int kt = 0; kt < ktiles; ++kt)
                for (int kq = 0; kq < 4; ++kq) {
                    half_t* hi = dst + ((((size_t)rt * ktiles + kt) * 2) * 64 + i + 16 * kq) * EPL;      // head fragment of the (tile, k-tile) pair; the tail 64 lanes behind it
                    half_t* lo = hi + 64 * EPL;
                    const int k0 = kt * KT + kq * EPL;
                    for (int j = 0; j < EPL; ++j) {
                        const float v = src ? CTTS_SPLIT_WSCALE * (colscale ? src[k0 + j] * colscale[k0 + j] : src[k0 + j]) : 0.f;      // the product rounds exactly like pack_tiles'
                        const half_t h = (half_t)v;
                        if (!(fabsf(v) <= 65504.0f)) in_range = false;
                        hi[j] = h;
                        lo[j] = (half_t)(v - (float)h);
                    }
                }
        }
    return in_range;
}

static const std::vector<float>* need(ctts_gpt* h, const std::string& k, size_t numel) {
    auto it = h->host.find(k);
    if (it == h->host.end()) { ctts_set_error("missing weight %s", k.c_str()); return nullptr; }
    if (it->second.size() != numel) { ctts_set_error("weight %s has %zu elements, expected %zu", k.c_str(), it->second.size(), numel); return nullptr; }
    return &it->second;
}

template <typename WT>
static int finalize_t(ctts_gpt* h) {
    const int H = h->H, I = h->I, L = h->L, V = h->V;
    const size_t n_qkv = (size_t)3 * H * H, n_o = (size_t)H * H, n_gu = (size_t)2 * I * H, n_d = (size_t)H * I;
    const int head_tiles = (h->NVQ * V + 15) / 16;
    const size_t n_head = (size_t)head_tiles * 16 * H;
    const size_t per_layer = n_qkv + n_o + n_gu + n_d;
    const size_t total = per_layer * L + n_head;
    std::vector<WT> blob(total);
    h->lw.resize(L);
    if (dev_alloc(h, (void**)&h->wblob, total * sizeof(WT))) return 1;
    // fp32 engine whose prompt passes can reach the split-GEMM threshold, or whose decode batches can reach split_decode_rows: head / tail fp16 images of the layer matrices too
    const bool want_split = (sizeof(WT) == 4) && (h->batch_inv || (h->split_rows_min > 0 && (long)h->cfg.max_batch * h->cfg.max_seq >= h->split_rows_min) ||
                                                   (h->split_dec_rows > 0 && h->cfg.max_batch >= h->split_dec_rows));
    std::vector<half_t> sblob;
    if (want_split) {
        sblob.resize(per_layer * 2 * L);
        if (dev_alloc(h, (void**)&h->wsplit, per_layer * L * 2 * sizeof(half_t))) return 1;
    }
    if (dev_alloc(h, (void**)&h->ln1, (size_t)L * H * 4)) return 1;       // input_layernorm weights, unfolded: the LoRA path needs w * x_hat itself
    struct LayerSrc { const std::vector<float>*q, *k, *v, *o, *g, *u, *d, *l1, *l2; };
    std::vector<LayerSrc> ls(L);
    for (int l = 0; l < L; ++l) {
        const std::string p = "gpt.layers." + std::to_string(l) + ".";
        LayerSrc& t = ls[l];
        t.q = need(h, p + "self_attn.q_proj.weight", n_o); t.k = need(h, p + "self_attn.k_proj.weight", n_o);
        t.v = need(h, p + "self_attn.v_proj.weight", n_o); t.o = need(h, p + "self_attn.o_proj.weight", n_o);
        t.g = need(h, p + "mlp.gate_proj.weight", (size_t)I * H); t.u = need(h, p + "mlp.up_proj.weight", (size_t)I * H);
        t.d = need(h, p + "mlp.down_proj.weight", n_d); t.l1 = need(h, p + "input_layernorm.weight", H);
        t.l2 = need(h, p + "post_attention_layernorm.weight", H);
        if (!t.q || !t.k || !t.v || !t.o || !t.g || !t.u || !t.d || !t.l1 || !t.l2) return 1;
        CTTS_HIP_CHECK(hipMemcpy(h->ln1 + (size_t)l * H, t.l1->data(), (size_t)H * 4, hipMemcpyHostToDevice));
        h->ln2_host.insert(h->ln2_host.end(), t.l2->begin(), t.l2->end());      // post_attention_layernorm weights, unfolded: uploaded with the first MLP target (lora_ensure_mlp_storage)
    }
    // host-side packing of the 20 layers on a few threads (pure CPU work on disjoint slices of the blobs)
    std::atomic<bool> split_in_range(true);
    auto pack_layer = [&](int l) {
        const LayerSrc& t = ls[l];
        const int HT = H / 16;
        auto qkv_row = [&](int pr) -> const float* {      // QKV: tile rows = dims [8t..8t+7 | 8t+32..8t+39] of one head, so RoPE's (d, d+32) pair sits in one tile
            const int rt = pr / 16, i = pr % 16;
            const int which = rt / HT, within = rt % HT, hh = within / 4, tq = within % 4;
            const int dd = (i < 8) ? 8 * tq + i : 8 * tq + (i - 8) + 32;
            const std::vector<float>* src = which == 0 ? t.q : (which == 1 ? t.k : t.v);
            return src->data() + (size_t)(hh * CTTS_HEAD_DIM + dd) * H;
        };
        auto o_row = [&](int pr) { return t.o->data() + (size_t)pr * H; };
        auto gu_row = [&](int pr) -> const float* {       // gate|up: tile rows = [8 gate rows | the matching 8 up rows]
            const int rt = pr / 16, i = pr % 16;
            return (i < 8) ? t.g->data() + (size_t)(rt * 8 + i) * H : t.u->data() + (size_t)(rt * 8 + i - 8) * H;
        };
        auto d_row = [&](int pr) { return t.d->data() + (size_t)pr * I; };
        WT* base = blob.data() + per_layer * l;
        // RMSNorm weights folded into the columns: W (w * xn) == (W diag(w)) xn  (llama.py:87,619-621)
        pack_tiles<WT>(base, 3 * HT, H, qkv_row, t.l1->data());
        pack_tiles<WT>(base + n_qkv, HT, H, o_row);
        pack_tiles<WT>(base + n_qkv + n_o, 2 * I / 16, H, gu_row, t.l2->data());
        pack_tiles<WT>(base + n_qkv + n_o + n_gu, HT, I, d_row);
        if (want_split) {
            half_t* sp = sblob.data() + per_layer * 2 * l;
            bool ok = pack_tiles_split(sp, 3 * HT, H, qkv_row, t.l1->data());
            ok = pack_tiles_split(sp + 2 * n_qkv, HT, H, o_row) && ok;
            ok = pack_tiles_split(sp + 2 * (n_qkv + n_o), 2 * I / 16, H, gu_row, t.l2->data()) && ok;
            ok = pack_tiles_split(sp + 2 * (n_qkv + n_o + n_gu), HT, I, d_row) && ok;
            if (!ok) split_in_range.store(false);
        }
    };
    {
        const int nthreads = L < 8 ? L : 8;
        std::vector<std::thread> pool;
        for (int w = 0; w < nthreads; ++w)
            pool.emplace_back([&, w]() { for (int l = w; l < L; l += nthreads) pack_layer(l); });
        for (auto& th : pool) th.join();
    }
    for (int l = 0; l < L; ++l) {
        char* dv = h->wblob + per_layer * l * sizeof(WT);
        h->lw[l].qkv = dv;
        h->lw[l].o = dv + n_qkv * sizeof(WT);
        h->lw[l].gu = dv + (n_qkv + n_o) * sizeof(WT);
        h->lw[l].d = dv + (n_qkv + n_o + n_gu) * sizeof(WT);
        if (want_split) {
            char* sv = h->wsplit + per_layer * l * 2 * sizeof(half_t);
            h->lw[l].qkv_sp = sv;
            h->lw[l].o_sp = sv + n_qkv * 4;
            h->lw[l].gu_sp = sv + (n_qkv + n_o) * 4;
            h->lw[l].d_sp = sv + (n_qkv + n_o + n_gu) * 4;
        }
    }
    if (want_split) CTTS_HIP_CHECK(hipMemcpy(h->wsplit, sblob.data(), sblob.size() * sizeof(half_t), hipMemcpyHostToDevice));
    h->split_ok = want_split && split_in_range.load();
    if (want_split && !h->split_ok) { h->split_rows_min = 0; h->split_dec_rows = 0; }      // a weight beyond +-1023: the head / tail images would hold inf -- this engine keeps the exact fp32 kernels
    // heads: fold weight norm, W = v * (g / ||v||_row)  (gpt.py:57-77; torch._weight_norm dim=0)
    std::vector<float> folded((size_t)h->NVQ * V * H);
    for (int i = 0; i < h->NVQ; ++i) {
        const std::string p = "head_code." + std::to_string(i) + ".parametrizations.weight.original";
        const std::vector<float>*g0 = need(h, p + "0", V), *v1 = need(h, p + "1", (size_t)V * H);
        if (!g0 || !v1) return 1;
        for (int r = 0; r < V; ++r) {
            double ss = 0.0;
            const float* vr = v1->data() + (size_t)r * H;
            for (int c = 0; c < H; ++c) ss += (double)vr[c] * vr[c];
            const float a = (*g0)[r] / (float)sqrt(ss);
            float* dst = folded.data() + ((size_t)i * V + r) * H;
            for (int c = 0; c < H; ++c) dst[c] = vr[c] * a;
        }
    }
    const int nvalid = h->NVQ * V;
    const std::vector<float>* nf = need(h, "gpt.norm.weight", H);
    if (!nf) return 1;
    pack_tiles<WT>(blob.data() + per_layer * L, head_tiles, H, [&](int pr) -> const float* {
        return pr < nvalid ? folded.data() + (size_t)pr * H : nullptr;
    }, nf->data());
    h->whead = h->wblob + per_layer * L * sizeof(WT);
    if (h->split_ok && (h->split_dec_rows > 0 || h->batch_inv)) {      // the code heads' split images (the decode path's last projection)
        std::vector<half_t> hs((size_t)head_tiles * 16 * H * 2);
        const bool ok = pack_tiles_split(hs.data(), head_tiles, H, [&](int pr) -> const float* { return pr < nvalid ? folded.data() + (size_t)pr * H : nullptr; }, nf->data());
        if (ok) {
            if (dev_alloc(h, &h->whead_sp, hs.size() * sizeof(half_t))) return 1;
            CTTS_HIP_CHECK(hipMemcpy(h->whead_sp, hs.data(), hs.size() * sizeof(half_t), hipMemcpyHostToDevice));
        }
    }
    {   // refine-text head (gpt.py:57-64): same weight-norm fold + final-norm fold, its own allocation
        auto g0 = h->host.find("head_text.parametrizations.weight.original0");
        auto v1 = h->host.find("head_text.parametrizations.weight.original1");
        if (g0 != h->host.end() && v1 != h->host.end() && v1->second.size() == g0->second.size() * (size_t)H) {
            const int Vt = (int)g0->second.size(), tiles = (Vt + 15) / 16;
            std::vector<float> ft((size_t)Vt * H);
            for (int r = 0; r < Vt; ++r) {
                double ss = 0.0;
                const float* vr = v1->second.data() + (size_t)r * H;
                for (int c = 0; c < H; ++c) ss += (double)vr[c] * vr[c];
                const float a = g0->second[r] / (float)sqrt(ss);
                for (int c = 0; c < H; ++c) ft[(size_t)r * H + c] = vr[c] * a;
            }
            std::vector<WT> packed((size_t)tiles * 16 * H);
            pack_tiles<WT>(packed.data(), tiles, H, [&](int pr) -> const float* { return pr < Vt ? ft.data() + (size_t)pr * H : nullptr; }, nf->data());
            if (dev_alloc(h, &h->whead_text, packed.size() * sizeof(WT))) return 1;
            CTTS_HIP_CHECK(hipMemcpy(h->whead_text, packed.data(), packed.size() * sizeof(WT), hipMemcpyHostToDevice));
            h->vocab_text_head = Vt;
        }
    }
    CTTS_HIP_CHECK(hipMemcpy(h->wblob, blob.data(), total * sizeof(WT), hipMemcpyHostToDevice));
    if (dev_alloc(h, (void**)&h->lnf, H * 4)) return 1;
    CTTS_HIP_CHECK(hipMemcpy(h->lnf, nf->data(), H * 4, hipMemcpyHostToDevice));
    if (dev_alloc(h, (void**)&h->emb_code, (size_t)h->NVQ * V * H * 4)) return 1;
    for (int i = 0; i < h->NVQ; ++i) {
        const std::vector<float>* e = need(h, "emb_code." + std::to_string(i) + ".weight", (size_t)V * H);
        if (!e) return 1;
        CTTS_HIP_CHECK(hipMemcpy(h->emb_code + (size_t)i * V * H, e->data(), (size_t)V * H * 4, hipMemcpyHostToDevice));
    }
    return 0;
}

extern "C" int ctts_gpt_finalize(ctts_gpt* h) {
    if (!h) { ctts_set_error("null handle"); return 1; }
    if (h->finalized) return 0;
    int rc = (h->cfg.dtype == CTTS_DTYPE_F16) ? finalize_t<half_t>(h) : finalize_t<float>(h);
    if (rc) return rc;
    const int H = h->H, NH = h->NH, MB = h->cfg.max_batch;
    {   // prompt rows per pass: never more than the engine can hold at all
        long cap = (long)MB * h->cfg.max_seq;
        cap = (cap + 255) / 256 * 256;
        h->pass_rows = (int)(cap < PASS_ROWS_MAX ? cap : PASS_ROWS_MAX);
        if (const char* pr = getenv("CTTS_PASS_ROWS")) { const int v = atoi(pr); if (v >= 256 && v < h->pass_rows) h->pass_rows = v / 256 * 256; }
    }
    const int PASS_ROWS = h->pass_rows;
    const size_t act_bytes = (size_t)((PASS_ROWS + PASS_PAD) / 16) * (h->I / (h->esz == 2 ? 32 : 16)) * 1024;
    if (dev_alloc(h, (void**)&h->x_dec, (size_t)CTTS_MAX_B * H * 4) || dev_alloc(h, (void**)&h->x_last, (size_t)CTTS_MAX_B * H * 4) ||
        dev_alloc(h, (void**)&h->x_pre, (size_t)PASS_ROWS * H * 4) ||
        dev_alloc(h, (void**)&h->q_buf, (size_t)PASS_ROWS * H * 4) ||
        dev_alloc(h, (void**)&h->part_ml, (size_t)(CTTS_MAX_B + 32) * NH * SMAX * 2 * 4) ||          // flash-decoding partials: decode rows only (the prompt pass never splits keys)
        dev_alloc(h, (void**)&h->part_o, (size_t)(CTTS_MAX_B + 32) * NH * SMAX * CTTS_HEAD_DIM * 4) ||
        dev_alloc(h, (void**)&h->logits, (size_t)CTTS_MAX_B * (h->NVQ * h->V > h->vocab_text_head ? h->NVQ * h->V : h->vocab_text_head) * 4) || dev_alloc(h, &h->act, act_bytes) || dev_alloc(h, (void**)&h->rope_pre, (size_t)MB * h->cfg.max_seq * 64 * 4) ||
        dev_alloc(h, (void**)&h->rope_dec, (size_t)CTTS_MAX_B * 64 * 4) || dev_alloc(h, (void**)&h->dpart, (size_t)32 * 4 * H * 4) || dev_alloc(h, &h->attn_packed, (size_t)((PASS_ROWS + PASS_PAD) / 16) * (H / (h->esz == 2 ? 32 : 16)) * 1024) ||
        dev_alloc(h, &h->norm_packed, (size_t)((PASS_ROWS + PASS_PAD) / 16) * (H / (h->esz == 2 ? 32 : 16)) * 1024) ||
        dev_alloc(h, (void**)&h->meta_pre, (size_t)MB * h->cfg.max_seq * sizeof(RowMeta)) ||
        dev_alloc(h, (void**)&h->meta_dec, CTTS_MAX_B * sizeof(RowMeta)) || dev_alloc(h, (void**)&h->meta_dec0, CTTS_MAX_B * sizeof(RowMeta)) ||
        dev_alloc(h, (void**)&h->st, sizeof(DevState)) || dev_alloc(h, (void**)&h->last_rows, CTTS_MAX_B * 4) ||
        dev_alloc(h, (void**)&h->dyn, sizeof(SamplerDyn)) || dev_alloc(h, (void**)&h->hist_ring, (size_t)CTTS_MAX_B * CTTS_NUM_VQ * 16 * 4) ||
        dev_alloc(h, (void**)&h->finend, (size_t)CTTS_MAX_B * (sizeof(RowState) + sizeof(RowSampling))) || dev_alloc(h, (void**)&h->sat, 4) ||
        dev_alloc(h, (void**)&h->cknobs, (size_t)CTTS_MAX_B * sizeof(RowSampling)) ||
        dev_alloc(h, (void**)&h->sk_slab, (size_t)(H / 16) * (CTTS_MAX_B / 16) * 4 * 256 * 4) || dev_alloc(h, (void**)&h->sk_cnt, (size_t)(H / 16) * (CTTS_MAX_B / 16) * 4) ||
        dev_alloc(h, (void**)&h->cx, (size_t)CTTS_MAX_B * H * 4) || dev_alloc(h, (void**)&h->crope, (size_t)CTTS_MAX_B * 64 * 4) ||
        dev_alloc(h, (void**)&h->cmeta, CTTS_MAX_B * sizeof(RowMeta)) || dev_alloc(h, (void**)&h->cring, (size_t)CTTS_MAX_B * CTTS_NUM_VQ * 16 * 4) ||
        dev_alloc(h, (void**)&h->cfin, (size_t)CTTS_MAX_B * sizeof(RowState)) || dev_alloc(h, (void**)&h->keep_dev, CTTS_MAX_B * 4) ||
        dev_alloc(h, &h->xh, (size_t)((CTTS_MAX_B + 32) / 16) * (H / (h->esz == 2 ? 32 : 16)) * 1024) || dev_alloc(h, (void**)&h->ssq, (size_t)(CTTS_MAX_B + 32) * (H / 16) * 4) ||
        dev_alloc(h, (void**)&h->scale_o, (size_t)(CTTS_MAX_B + 32) * 4) || dev_alloc(h, (void**)&h->scale_d, (size_t)(CTTS_MAX_B + 32) * 4) ||
        dev_alloc(h, (void**)&h->rope_dec0, (size_t)CTTS_MAX_B * 64 * 4))
        return 1;
    if (h->wsplit) {     // operand images of the prompt rows for the split GEMMs: heads / tails of the normalised rows | attention outputs (K = 768) and of the SwiGLU outputs (K = 3072)
        const size_t rows = (size_t)PASS_ROWS + PASS_PAD;
        if (dev_alloc(h, &h->sp_x_hi, rows * H * 2) || dev_alloc(h, &h->sp_x_lo, rows * H * 2) || dev_alloc(h, &h->sp_act_hi, rows * h->I * 2) || dev_alloc(h, &h->sp_act_lo, rows * h->I * 2)) return 1;
        // short passes slice the down projection's K four ways (prefill_split.hip sp_launch): the slices' partial outputs [4][rows <= 2048, padded to 128][H] fp32 (<= 25 MB)
        h->sk_cap_floats = (size_t)4 * (size_t)(((PASS_ROWS < 2048 ? PASS_ROWS : 2048) + 127) / 128 * 128) * H;
        if (dev_alloc(h, (void**)&h->sk_scratch, h->sk_cap_floats * 4)) return 1;
    }
    h->knobs = (RowSampling*)(h->finend + CTTS_MAX_B);      // (the sampler derives this address from its finend argument)
    CTTS_HIP_CHECK(hipHostMalloc((void**)&h->host_pin, 64));
    {
        auto it = h->host.find("emb_text.weight");
        if (it != h->host.end() && it->second.size() % H == 0) {
            h->vocab_text = (int)(it->second.size() / H);
            if (dev_alloc(h, (void**)&h->emb_text, it->second.size() * 4)) return 1;
            CTTS_HIP_CHECK(hipMemcpy(h->emb_text, it->second.data(), it->second.size() * 4, hipMemcpyHostToDevice));
        }
    }
    if (h->whead_text && h->emb_text && h->vocab_text_head > h->vocab_text) {
        // the text sampler re-embeds any sampled id < vocab_text_head through emb_text: a larger head would read past the table
        ctts_set_error("finalize: head_text has %d rows but emb_text only %d", h->vocab_text_head, h->vocab_text);
        return 1;
    }
    h->host.clear();
    h->finalized = true;
    if (h->persist_rows > 0 && ensure_persist(h, false)) return 1;
    return 0;
}

extern "C" int ctts_gpt_embed(ctts_gpt* h, const int32_t* ids, const int32_t* text_mask, int B, int T, const float* spk, int spk_id, float* emb_out, void* stream) {
    if (!h || !h->finalized || !ids || !text_mask || !emb_out || B < 1 || T < 1) { ctts_set_error("embed: bad argument"); return 1; }
    if (!h->emb_text) { ctts_set_error("embed: emb_text.weight was not loaded"); return 1; }
    return launch_embed_prompt(ids, text_mask, h->emb_text, h->emb_code, spk, spk_id, emb_out, B * T, T, h->V, h->H, (hipStream_t)stream);
}

extern "C" size_t ctts_gpt_kv_bytes(const ctts_gpt* h) {
    return (size_t)h->L * 2 * h->cfg.max_batch * h->NH * h->cfg.max_seq * CTTS_HEAD_DIM * h->esz;
}
extern "C" int ctts_gpt_bind_kv(ctts_gpt* h, void* kv, size_t bytes) {
    if (!h || !kv || bytes < ctts_gpt_kv_bytes(h)) { ctts_set_error("bind_kv: need %zu bytes", h ? ctts_gpt_kv_bytes(h) : 0); return 1; }
    h->kv = (char*)kv; h->kv_bytes = bytes;
    // graphs are keyed by the KV pointer; entries captured against an older binding are simply never selected again
    return 0;
}
extern "C" int ctts_gpt_set_rope(ctts_gpt* h, const float* rope_host, int n_pos) {
    if (!h || !rope_host || n_pos < h->cfg.max_seq) { ctts_set_error("set_rope: need at least max_seq=%d positions", h ? h->cfg.max_seq : 0); return 1; }
    dev_free(h, h->rope); h->rope = nullptr;
    if (dev_alloc(h, (void**)&h->rope, (size_t)(n_pos + 1) * 64 * 4)) return 1;   // +1: the sampler prefetches the row of the position after the last one
    CTTS_HIP_CHECK(hipMemcpy(h->rope, rope_host, (size_t)n_pos * 64 * 4, hipMemcpyHostToDevice));
    h->rope_n = n_pos;
    return 0;
}

// ---- launch sequencing -----------------------------------------------------------------------
static inline void* kv_layer(ctts_gpt* h, int l, int which) {
    const size_t per = (size_t)h->cfg.max_batch * h->NH * h->cfg.max_seq * CTTS_HEAD_DIM * h->esz;
    return h->kv + ((size_t)l * 2 + which) * per;
}
// The row-count thresholds the launches use.  "batch_invariant" pins every choice that depends on the row count, the pass height or the padding, and THIS is where: no
// persistent launch, no VALU rows, the split projections from 1 row on (one padded 16-row chunk), the down projection's K sliced inside the launch and never by launch slices,
// never 32-row blocks at decode, unsplit attention on 8-wave blocks, the prompt's K never sliced (ctts_gpt_begin refuses adapters then).  plan_layers adds the two choices that are no threshold.
// The same pins serve fp16 engines ("schedule_invariant"): split_dec_rows / valu_rows / split_nbg2_rows name fp32 mechanisms and are simply never consulted there, the rest puts every row
// count on the packed-residual chain (xhm) in 16-row chunks with EPI_RESID_XH_SK; the weight-prefetch workgroups keep their own threshold (17 rows): they do no arithmetic.
struct Tuning { bool inv; int persist_rows, valu_rows, split_dec_rows, split_rows, down_sk_rows, nbg2_rows, split_nbg2_rows, force_splits, attn_wide_blocks, prefill_sk_rows; };
static inline Tuning tuning(const ctts_gpt* h) {
    if (h->batch_inv) return {true, 0, 0, 1, 0, 1, OPT_MAX, OPT_MAX, 1, OPT_MAX, 0};
    return {false, h->persist_rows, h->valu_rows, h->split_dec_rows, h->split_rows, h->down_sk_rows, h->nbg2_rows, h->split_nbg2_rows, h->force_splits, h->attn_wide_blocks, h->prefill_sk_rows};
}
// the persistent weight images, built lazily before the first step that could use them is planned (outside capture: see persist_images)
static int ensure_persist_images(ctts_gpt* h) {
    const int rows = tuning(h).persist_rows;
    return (h->persist_ok && h->pimg == nullptr && rows > 0 && h->B <= rows && (!h->lora_rows || h->persist_lora)) ? persist_images(h) : 0;
}

// Key splits of the decode attention for a batch of B rows whose longest context in the coming steps is L keys.
// Cap: enough (row, head, split) blocks to cover the chip.  Measured (us/step, 256 steps from a 48-token prompt unless noted):
//   B=1: S=1 412, 2 400, 4 392, 8 392;  L~1900: S=1 628, 2 589, 8 438        -> one row: always the cap
//   B=4: S=1 438, 2 456, 4 449;  B=8: S=1 476, 2 535                          -> S > 1 pays a softmax-combine prologue per row
// in o_proj (S = 1 lets the attention write o_proj's packed operand directly): from 4 rows on, split only when one
// 8-wave block would otherwise loop over more than ~768 keys.
static inline int decode_splits(const ctts_gpt* h, int B, int L) {
    const int forced = tuning(h).force_splits;             // (batch_invariant: 1 -- a function of neither the batch nor the longest row)
    if (h->lora_rows) return 1;                            // per-utterance LoRA reads the attention output from o_proj's packed operand (S = 1 path)
    if (forced) return forced;
    int cap = 256 / (B * h->NH);
    cap = cap < 1 ? 1 : (cap > SMAX ? SMAX : cap);
    if (B <= 2) return cap;
    if (B >= 8) return 1;                                  // B=8, L 1200..1700: S=1 703, S=2 746
    const int want = (L + 767) / 768;
    return want < 1 ? 1 : (want > cap ? cap : want);
}

// How run_layers leaves the residual stream to whatever reads it next (the heads), and the heads' launch shape: one place computes the predicates, the consumer
// uses what was actually launched.  parts: x = x_dec + dpart[0..3] (split-K down projection) / xh: packed copy + sums of squares exist / logits: the logits (and
// hidden rows) exist already / split: the packed copy is a head / tail fp16 pair (split_t) / nbg, valu: the heads' block height (16 * nbg rows) and VALU form
struct StreamForm { bool parts, xh, logits, split; int nbg, valu; };
// decode rows per block / 16: see nbg2_rows / split_nbg2_rows (`split`: the projections read head / tail images)
static inline int decode_nbg(const Tuning& t, int R, bool split) { return (R <= 16 || R < (split ? t.split_nbg2_rows : t.nbg2_rows)) ? 1 : 2; }
// the heads' block height is a function of B and of whether the packed copy is a head / tail pair (the packed rows' layout does not depend on the producer's block height)
static StreamForm stream_form(const ctts_gpt* h, bool parts, bool xh, bool logits, bool split) {
    const Tuning t = tuning(h);
    return {parts, xh, logits, split, decode_nbg(t, h->B, split), (h->cfg.dtype == CTTS_DTYPE_F32 && h->B <= t.valu_rows) ? 1 : 0};
}
static inline StreamForm plain_form(const ctts_gpt* h) { return stream_form(h, false, false, false, false); }      // after a prompt pass / a restart: fp32 rows in x_dec

// Everything run_layers decides before its layer loop, for R rows of a decode step (`decode`, on path `path`) or of a prompt pass: computed once per call by
// plan_layers, which has no other effect; run_layers then only fills argument structs and launches.
struct LayerPlan {
    bool lora, lmlp;                  // per-utterance adapters: the residual stream must be materialised in x (no split-K partials) / ... on gate / up / down too: their terms come from two more lora.hip launches per layer, decode and prompt pass alike
    int S, nbg, chunks, dts, pf_kb, valu, wide_blocks, anchor, prefill_sk_rows;      // key splits; 16 * nbg rows per block, blocks; launch_gemm's operand format; see plan_layers for the rest
    int pfg_shape;                    // block shape of prefill_gemm.hip (-1 = by pass height)
    bool splitd, prepack, pfg, pfs, xhm, spd, down_sk, fuse_heads;
    int persist, per, pace, poll, delay_act, delay_u;      // persistent launch: key shares (0 = the launch chain), layers per launch, and its row-count defaults resolved
    StreamForm form;
};
static LayerPlan plan_layers(const ctts_gpt* h, int R, bool decode, DecodePath path) {
    LayerPlan p = {};
    const Tuning t = tuning(h);
    const int dt = h->cfg.dtype;
    p.S = path.splits; p.lora = h->lora_rows != 0; p.lmlp = p.lora && h->lora_mlp != 0;
    // fp32 engines, decode batches of >= split_decode_rows rows: head / tail fp16 operands (the predicate is completed below; it needs the packed-residual path)
    const bool spd_ok = decode && dt == CTTS_DTYPE_F32 && h->xh_mode && h->split_ok && h->wsplit != nullptr && !p.lora && p.S == 1 &&
                        t.split_dec_rows > 0 && R >= t.split_dec_rows && R > t.split_rows;
    // invariant fp16 engines ("schedule_invariant"): ONE prompt arithmetic at every pass height, 1 row included -- norm_pack, then the LDS-staged GEMM of prefill_gemm.hip
    // (every output accumulated by one wave in k order, rows past the end clamped, operand buffers sized for whole blocks) on its 128 x 128 blocks
    const bool inv16 = t.inv && dt == CTTS_DTYPE_F16 && !decode;
    p.nbg = decode ? decode_nbg(t, R, spd_ok) : ((R <= 16 && !inv16) ? 1 : 2);      // (the prompt pass keeps 32-row blocks)
    p.chunks = (R + 16 * p.nbg - 1) / (16 * p.nbg);
    // small decode batches: the down projection is launched as 4 split-K slices (192 blocks instead of 48 x 1024 threads);
    // its partial sums dp[0..3] are added, in order, by the next consumers of the residual stream (QKV RMSNorm, o_proj
    // residual, final heads) -- deterministic, no atomics.  x itself is re-materialised by every o_proj.
    p.splitd = decode && (R <= t.split_rows) && (p.nbg == 1) && !p.lora;
    // prompt pass over more than a few chunks: normalise every row once (norm_pack_kernel) instead of in every GEMM block
    p.prepack = inv16 || (!decode && (p.nbg == 2) && (R > 64) && !h->no_prepack);
    // prompt pass over >= 1536 rows, fp16: LDS-staged 256/128 x 128 MFMA GEMM (prefill_gemm.hip) instead of one weight tile per 32-row block
    // (measured with 128 x 128 blocks, prompt pass ms with / without it: 512 rows 2.31 / 1.48, 1024 rows 2.47 / 2.29, 1536 rows 2.70 / 3.12,
    //  2048 rows 2.81 / 3.9, 3072 rows 3.6 / 5.3, 16384 rows 10.3 / 29)
    p.pfg = inv16 || (p.prepack && (dt == CTTS_DTYPE_F16) && h->prefill_gemm_rows > 0 && (R >= h->prefill_gemm_rows) && !p.lora);
    p.pfg_shape = inv16 ? 0 : -1;
    // prompt pass over >= 384 rows, fp32 engine: the same tiling on the fp16 pipes with head / tail operands -- 3 MFMAs per product instead of 16,
    // fp32-level accuracy (prefill_split.hip); the attention stays the fp32 row kernel
    // (round 5: also with per-utterance adapters -- their low-rank terms come from the two lora.hip launches per layer and are added in the split GEMMs' epilogues)
    // (... and with adapters on gate / up / down: two more launches; the gate / up term rides in a SwiGLU epilogue of its own, the down term is read from the act images)
    // (invariant: every pass height, 1 row included -- the block shapes give bit-identical rows, tools/prefill_fuzz.py -- and the down projection's K never sliced)
    p.pfs = (dt == CTTS_DTYPE_F32) && h->wsplit != nullptr &&
            (t.inv ? (!decode && h->split_ok) : (p.prepack && h->split_rows_min > 0 && (R >= h->split_rows_min)));
    // decode above the split-K batch sizes: the residual stream travels between kernels as a packed B operand in the engine dtype + per-tile
    // sums of squares (EPI_RESID_XH -> PRO_XH, kernels.h); layer 0 still normalises the sampler's fp32 rows itself.  (Handing gate|up
    // the packed copy at batches <= 4 too was measured slower in fp16: batch 1 393 vs 381 us/step, 2 415 vs 403, 4 450 vs 443.)
    // fp32: the RMSNorm factor then multiplies the C tile instead of the operand -- (sum w x) rs instead of sum w (x rs), one rounding
    // apart; token ids stay bit-exact on every golden (tests/test_gpu_gpt.py)
    p.xhm = decode && h->xh_mode && !p.splitd;
    // ... and from split_decode_rows rows on (fp32 engines) the projections read head / tail fp16 images of weights and operands: 3 fp16 MFMAs per product instead of 8
    // exact-f32 ones (common.h split_t; the prompt pass's arithmetic, prefill_split.hip).  Layer 0's q|k|v projection normalises the sampler's fp32 rows and stays exact.
    p.spd = p.xhm && spd_ok;
    p.dts = p.spd ? 2 : dt;
    // weight prefetch across a launch boundary of a decode step (kernels.h WPrefetch): the o_proj launch carries workgroups that pull the gate|up launch's weight image into L2
    // (packed-residual path: every consumer workgroup column is one row tile; per-utterance adapters shift the consumers' block indices by their workers: off)
    p.pf_kb = (p.xhm && !p.lora && (p.spd || (dt == CTTS_DTYPE_F16 && R >= 17))) ? h->prefetch_kb : 0;      // (the exact-f32 kernels lose with it: batch 32 0.845 -> 0.897)
    p.valu = (decode && dt == CTTS_DTYPE_F32 && R <= t.valu_rows && !p.lora) ? 1 : 0;
    // the packed-residual down projection with its K sliced 4 ways inside the launch, last arriver combines (EPI_RESID_XH_SK, kernels.h): see down_sk_rows
    p.down_sk = (p.nbg == 1 || p.spd) && R >= t.down_sk_rows && t.down_sk_rows > 0;
    p.wide_blocks = t.attn_wide_blocks; p.anchor = t.inv ? 1 : 0; p.prefill_sk_rows = t.prefill_sk_rows;
    p.form = stream_form(h, p.splitd, p.xhm, false, p.spd);
    // one persistent launch per layer (persist_layer.hip): the residual stream stays in x, nothing is left in partial or packed form
    p.persist = (decode && h->pimg != nullptr && R <= PL_MAXR) ? path.persist : 0;
    if (p.persist) {
        // the launch that ends the stack also runs the final norm + the 4 code heads (persist_layer.hip phase H): code mode, paced schedule, images built
        // (ms/step separate heads launch / fused, tools/ab_options.py: fp32 batch 1 0.2798 / 0.2786, 2 0.3396 / 0.3384, 4 0.4711 / 0.4721; fp16 batch 3 0.3793 / 0.3800 -> up to 2 rows)
        // (not in a mixed step, text rows beside code rows: the fused heads read the stack's output from the launch's granules and leave x_dec at the stack's INPUT --
        //  the text head of a mixed step reads x_dec, so such a step ends with the separate heads launches)
        p.fuse_heads = h->persist_heads && R <= 2 && !h->text_mode && h->text_live == 0 && h->persist_sched == 3 && h->pimg_head != nullptr && h->dyn != nullptr;
        p.form = stream_form(h, false, false, p.fuse_heads, false);
        // (persistent_layers_per_launch, default all: the whole stack is ONE launch; 1 = a launch per layer, the first version of the structure)
        p.per = (h->persist_lpl > 0 && h->persist_lpl < h->L) ? h->persist_lpl : h->L;
        p.pace = h->persist_pace < 0 ? (R <= 2 ? 3 : 2) : h->persist_pace; p.poll = (h->persist_poll < 0) ? 0 : h->persist_poll;
        p.delay_act = h->persist_delay_act + 2 * (R - 1); p.delay_u = h->persist_delay_u < 0 ? 14 + 2 * R : h->persist_delay_u;
    }
    return p;
}

// 20 decoder layers on R rows of residual stream x (llama.py:719-749 per layer); st != nullptr: a decode step on `path`, else a prompt pass ({1, 0}) over rows of
// T_rows tokens per sequence (prompt_passes)
static int run_layers(ctts_gpt* h, float* x, const RowMeta* meta, const float* rope_rows, int R, DecodePath path, const DevState* st, hipStream_t s, StreamForm* form = nullptr, int T_rows = 0) {
    const LayerPlan p = plan_layers(h, R, st != nullptr, path);
    const int dt = h->cfg.dtype, S = p.S, nbg = p.nbg, NB = 16 * nbg, chunks = p.chunks, dts = p.dts;
    const bool lora = p.lora, lmlp = p.lmlp, splitd = p.splitd, prepack = p.prepack, pfg = p.pfg, pfs = p.pfs, xhm = p.xhm, spd = p.spd;
    if (form) *form = p.form;
    if (p.persist) {
        for (int l = 0; l < h->L; l += p.per) {
            PersistArgs pa = {};
            if (p.fuse_heads && l + p.per >= h->L) {
                pa.heads = 1; pa.hw = h->pimg_head; pa.logits = h->logits; pa.n_valid = h->NVQ * h->V; pa.lnf = h->lnf; pa.dyn = h->dyn; pa.rows = h->finend;
            }
            pa.w = h->pimg + PL_LAYER_BYTES / 4 * h->esz * l; pa.half_w = h->esz == 2 ? 1 : 0; pa.n_layers = (h->L - l < p.per) ? h->L - l : p.per;
            pa.x = x; pa.meta = meta; pa.rope_rows = rope_rows;
            pa.kv = kv_layer(h, l, 0); pa.kv_per = (size_t)h->cfg.max_batch * h->NH * h->cfg.max_seq * CTTS_HEAD_DIM; pa.Lmax = h->cfg.max_seq;
            pa.g_qkv = h->pl_g; pa.g_att = pa.g_qkv + PL_G_QKV; pa.g_x1 = pa.g_att + PL_G_ATT; pa.g_act = pa.g_x1 + PL_G_X1; pa.g_x = pa.g_act + PL_G_ACT; pa.g_part = pa.g_x + PL_G_X; pa.S = p.persist;
            pa.epoch = h->pl_epoch; pa.error = h->pl_error; pa.done = &st->all_done; pa.ts = h->pl_ts_on ? h->pl_ts : nullptr; pa.eps = 1e-6f; pa.sched = h->persist_sched; pa.pace = p.pace; pa.fault = h->persist_fault; pa.delay_att = h->persist_delay_att; pa.delay = h->persist_delay; pa.delay_act = p.delay_act; pa.delay_x = h->persist_delay_x; pa.nap = h->persist_nap; pa.nap_qkv = h->persist_nap_qkv; pa.poll = p.poll;
            if (lora) {
                // per-utterance adapters: the rows' slots travel in the arguments (part of the decode-graph key), the operands are read from the resident tables
                pa.lora = 1; pa.delay_u = p.delay_u; static_assert(sizeof(pa.lslots) == PL_MAXR, "PersistArgs.lslots: byte r = row r's slot");
                row_slot_bytes(h, (signed char*)&pa.lslots, PL_MAXR);
                pa.la_qkv_stride = (size_t)CTTS_MAX_ADAPTERS * 3 * 16 * h->H; pa.la_stride = (size_t)CTTS_MAX_ADAPTERS * 4 * 16 * h->H;
                pa.la_qkv = h->lora_Af + pa.la_qkv_stride * l; pa.la = h->lora_A + pa.la_stride * l; pa.lb = h->lora_B + pa.la_stride * l;
                pa.lscale = h->lora_scale + (size_t)l * CTTS_MAX_ADAPTERS * 4; pa.g_u = pa.g_part + PL_G_PART;
            }
            if (launch_persist_layer(R, pa, s)) return 1;
        }
        return 0;
    }
    const float sp_scale = 1.0f / 64.0f;
    const SplitGemmPolicy sp_pol = {h->prefill_pp_blocks, p.prefill_sk_rows, h->sk_scratch, h->sk_cap_floats, h->prefill_small_blocks, h->prefill_ring4_blocks};
    auto set_pf = [&](GemmArgs& g, const void* w, int n_tiles, int K, int fmt) {          // fmt: 0 fp32 tiles, 1 fp16 tiles, 2 head / tail pairs
        if (p.pf_kb <= 0 || w == nullptr) return;
        const size_t tile = (size_t)16 * K * (fmt == 1 ? 2 : 4);
        size_t nb = (tile * n_tiles + (size_t)p.pf_kb * 1024 - 1) / ((size_t)p.pf_kb * 1024);
        nb = (nb + 7) & ~(size_t)7;
        nb = nb < 8 ? 8 : (nb > 256 ? 256 : nb);
        g.pf.ptr = w; g.pf.unit_bytes = (unsigned)tile; g.pf.n_units = (unsigned)n_tiles; g.pf_blocks = (int)nb;
    };
    if (lmlp && (h->lora_dgu == nullptr || h->lora_mrank.empty())) { ctts_set_error("per-utterance LoRA: the MLP targets' buffers are missing"); return 1; }
    for (int l = 0; l < h->L; ++l) {
        GemmArgs a = {};
        a.st = st; a.R = R; a.eps = 1e-6f; a.meta = meta; a.Lmax = h->cfg.max_seq; a.sat = h->sat;
        a.valu = p.valu;
        // RMSNorm + QKV + RoPE + KV append
        GemmArgs g1 = a;
        g1.W = h->lw[l].qkv; g1.n_row_tiles = 3 * h->H / 16; g1.K = h->H; g1.x = x;
        g1.q_out = h->q_buf; g1.k_cache = kv_layer(h, l, 0); g1.v_cache = kv_layer(h, l, 1); g1.rope_rows = rope_rows;
        g1.opart = h->dpart; g1.np = (splitd && l > 0) ? 4 : 0;
        const size_t lora_l = (size_t)l * CTTS_MAX_ADAPTERS * 4 * 16 * h->H;
        // decode steps: the rows' low-rank terms come from worker workgroups inside the QKV / o_proj launches (lora_worker.h) instead of two more launches
        const bool lfold = lora && st != nullptr && h->lora_fold && h->lora_g != nullptr && h->H == 768 && R <= CTTS_MAX_B;
        if (lfold) {
            LoraFold lf = {};
            lf.A = h->lora_A + lora_l; lf.B = h->lora_B + lora_l; lf.scale = h->lora_scale + (size_t)l * CTTS_MAX_ADAPTERS * 4; lf.lnw = h->ln1 + (size_t)l * h->H;
            row_slot_bytes(h, lf.slots, CTTS_MAX_B); static_assert(sizeof(lf.ranks) == CTTS_MAX_ADAPTERS * 4, "LoraFold.ranks");
            if (!h->lora_rank.empty()) memcpy(lf.ranks, &h->lora_rank[(size_t)l * CTTS_MAX_ADAPTERS * 4], sizeof(lf.ranks));
            lf.g = h->lora_g; lf.g_o = h->lora_g + (size_t)CTTS_MAX_B * 3 * h->H; lf.err = h->pl_error; lf.layer = l; lf.diag = h->lora_fold;
            g1.lf = lf; g1.lora_w = 3 * NB;
        } else if (lora) {
            if (launch_lora_delta_qkv(x, h->ln1 + (size_t)l * h->H, a.eps, meta, h->lora_slot_of_seq, h->lora_A + lora_l, h->lora_B + lora_l,
                                      h->lora_scale + (size_t)l * CTTS_MAX_ADAPTERS * 4, h->lora_dqkv, R, h->H, s)) return 1;
            g1.lora_delta = h->lora_dqkv;
        }
        if (pfs) {
            if (launch_norm_pack_split(x, h->sp_x_hi, h->sp_x_lo, R, a.eps, s)) return 1;
            if (launch_prefill_split_gemm(EPI_QKV, g1, h->lw[l].qkv_sp, h->sp_x_hi, h->sp_x_lo, nullptr, nullptr, sp_scale, sp_pol, s)) return 1;
        } else if (prepack) {
            g1.xpacked = h->norm_packed;
            if (launch_norm_pack(dt, x, h->norm_packed, R, nbg, a.eps, s)) return 1;
            if (pfg ? launch_prefill_gemm(EPI_QKV, g1, s, p.pfg_shape) : launch_gemm(dt, nbg, PRO_PACKED, EPI_QKV, g1, chunks, s)) return 1;
        } else if (xhm) {
            g1.scale_out = h->scale_o;
            if (l > 0) { g1.xh = h->xh; g1.ssq = h->ssq; g1.scale_in = h->scale_d; }
            if (spd && l > 0) g1.W = h->lw[l].qkv_sp;
            if (launch_gemm(l > 0 ? dts : dt, nbg, l > 0 ? PRO_XH : PRO_NORM, EPI_QKV, g1, chunks, s)) return 1;
        } else if (launch_gemm(dt, nbg, splitd ? PRO_NORM_P : PRO_NORM, EPI_QKV, g1, chunks, s)) return 1;
        AttnArgs at = {};
        at.q = h->q_buf; at.k_cache = g1.k_cache; at.v_cache = g1.v_cache; at.Lmax = h->cfg.max_seq; at.NH = h->NH; at.R = R; at.S = S;
        at.meta = meta; at.st = st; at.part_ml = h->part_ml; at.part_o = h->part_o; at.wide_blocks = p.wide_blocks; at.anchor = p.anchor;
        if (st == nullptr) { at.T = T_rows; at.row0 = (int)(meta - h->meta_pre); }       // prompt pass: position of this pass in the flattened [B][T] prompt
        at.packed_out = (S == 1) ? h->attn_packed : nullptr; at.nbg = nbg; at.packed_split = spd ? 1 : 0;
        if (prompt_attention_kind(dt, R, at.T, at.anchor, pfs && S == 1) == ATTN_SPLIT) { if (launch_attention_split(at, h->sp_x_hi, h->sp_x_lo, s)) return 1; }      // writes o_proj's head / tail operand images directly
        else if (launch_attention(dt, at, s)) return 1;
        // softmax combine + o_proj + residual (S == 1: attention already wrote the normalised, packed B operand)
        GemmArgs g2 = a;
        g2.W = h->lw[l].o; g2.n_row_tiles = h->H / 16; g2.K = h->H; g2.part_ml = h->part_ml; g2.part_o = h->part_o; g2.S = S; g2.x_out = x;
        g2.xpacked = h->attn_packed;
        g2.opart = h->dpart; g2.np = (splitd && l > 0) ? 4 : 0;      // the down projection's partial sums are folded into x here
        if (xhm) { g2.xh = h->xh; g2.ssq = h->ssq; g2.scale_in = h->scale_o; }
        if (lora && S != 1) { ctts_set_error("per-utterance LoRA needs unsplit attention"); return 1; }
        if (lfold) { g2.lf = g1.lf; g2.lora_w = NB; }
        else if (lora) {
            if (pfs && S == 1) {
                if (launch_lora_delta_o_split(h->sp_x_hi, h->sp_x_lo, meta, h->lora_slot_of_seq, h->lora_A + lora_l, h->lora_B + lora_l,
                                              h->lora_scale + (size_t)l * CTTS_MAX_ADAPTERS * 4, h->lora_do, R, h->H, s)) return 1;
            } else if (launch_lora_delta_o(dt, h->attn_packed, nbg, meta, h->lora_slot_of_seq, h->lora_A + lora_l, h->lora_B + lora_l,
                                           h->lora_scale + (size_t)l * CTTS_MAX_ADAPTERS * 4, h->lora_do, R, h->H, s)) return 1;
            g2.lora_delta = h->lora_do;
        }
        if (pfs && S == 1) {
            if (launch_prefill_split_gemm(EPI_RESID, g2, h->lw[l].o_sp, h->sp_x_hi, h->sp_x_lo, nullptr, nullptr, sp_scale, sp_pol, s)) return 1;
        } else if (pfg && S == 1) { if (launch_prefill_gemm(EPI_RESID, g2, s, p.pfg_shape)) return 1; }
        else {
            if (spd) g2.W = h->lw[l].o_sp;
            set_pf(g2, spd ? h->lw[l].gu_sp : h->lw[l].gu, 2 * h->I / 16, h->H, dts);
            if (launch_gemm(dts, nbg, (S == 1) ? PRO_PACKED : PRO_ATTN, xhm ? EPI_RESID_XH : (splitd ? EPI_RESID_P : EPI_RESID), g2, chunks, s)) return 1;
        }
        // RMSNorm + gate|up + SiLU*up
        GemmArgs g3 = a;
        g3.W = h->lw[l].gu; g3.n_row_tiles = 2 * h->I / 16; g3.K = h->H; g3.x = x; g3.act_out = h->act;
        const size_t mlp_l = (size_t)l * CTTS_MAX_ADAPTERS;
        if (lmlp) {       // gate / up terms of every row from the residual stream o_proj just completed; the SwiGLU epilogues add them before the activation
            if (launch_lora_delta_gu(x, h->ln2 + (size_t)l * h->H, a.eps, meta, h->lora_slot_of_seq, h->lora_mA_gu + mlp_l * 2 * 16 * h->H, h->lora_mB_gu + mlp_l * 2 * 16 * h->I,
                                     h->lora_mscale + mlp_l * 4, h->lora_dgu, R, h->H, h->I, s)) return 1;
            g3.lora_delta = h->lora_dgu; g3.lora_gu = 1;
        }
        if (pfs) {
            if (launch_norm_pack_split(x, h->sp_x_hi, h->sp_x_lo, R, a.eps, s)) return 1;
            if (launch_prefill_split_gemm(EPI_SWIGLU, g3, h->lw[l].gu_sp, h->sp_x_hi, h->sp_x_lo, h->sp_act_hi, h->sp_act_lo, sp_scale, sp_pol, s)) return 1;
        } else if (prepack) {
            g3.xpacked = h->norm_packed;
            if (launch_norm_pack(dt, x, h->norm_packed, R, nbg, a.eps, s)) return 1;
            if (pfg ? launch_prefill_gemm(EPI_SWIGLU, g3, s, p.pfg_shape) : launch_gemm(dt, nbg, PRO_PACKED, EPI_SWIGLU, g3, chunks, s)) return 1;
        } else if (xhm) {
            g3.xh = h->xh; g3.ssq = h->ssq; g3.scale_in = h->scale_o; g3.scale_out = h->scale_d;
            if (spd) g3.W = h->lw[l].gu_sp;
            if (launch_gemm(dts, nbg, PRO_XH, EPI_SWIGLU, g3, chunks, s)) return 1;
        } else if (launch_gemm(dt, nbg, PRO_NORM, EPI_SWIGLU, g3, chunks, s)) return 1;
        // down + residual
        GemmArgs g4 = a;
        g4.W = h->lw[l].d; g4.n_row_tiles = h->H / 16; g4.K = h->I; g4.xpacked = h->act; g4.x_out = x;
        if (lmlp) {       // down term from the operand the down projection itself reads (the packed SwiGLU output, or the split pass's head / tail images); added with the residual
            if (pfs ? launch_lora_delta_down_split(h->sp_act_hi, h->sp_act_lo, meta, h->lora_slot_of_seq, h->lora_mA_d + mlp_l * 16 * h->I, h->lora_mB_d + mlp_l * 16 * h->H,
                                                   h->lora_mscale + mlp_l * 4, h->lora_do, R, h->H, h->I, s)
                    : launch_lora_delta_down(dt, h->act, nbg, meta, h->lora_slot_of_seq, h->lora_mA_d + mlp_l * 16 * h->I, h->lora_mB_d + mlp_l * 16 * h->H,
                                             h->lora_mscale + mlp_l * 4, h->lora_do, R, h->H, h->I, s)) return 1;
            g4.lora_delta = h->lora_do;
        }
        if (pfs) {      // the SwiGLU images hold silu(g) * u / 16
            if (launch_prefill_split_gemm(EPI_RESID, g4, h->lw[l].d_sp, h->sp_act_hi, h->sp_act_lo, nullptr, nullptr, sp_scale * 16.0f, sp_pol, s)) return 1;
        } else if (pfg) {
            if (launch_prefill_gemm(EPI_RESID, g4, s, p.pfg_shape)) return 1;
        } else if (splitd) {
            g4.part_out = h->dpart; g4.ktiles_total = h->I / (h->esz == 2 ? 32 : 16);
            if (launch_gemm(dt, nbg, PRO_PACKED, EPI_PART, g4, chunks, s)) return 1;
        } else if (xhm) {                          // (the last layer's copy is for the heads: run_heads)
            g4.xh = h->xh; g4.ssq = h->ssq; g4.scale_in = h->scale_d;
            if (spd) g4.W = h->lw[l].d_sp;
            if (p.down_sk) {
                g4.ktiles_total = h->I / ((h->esz == 2 || spd) ? 32 : 16); g4.sk_slab = h->sk_slab; g4.sk_cnt = h->sk_cnt;
                if (launch_gemm(dts, nbg, PRO_PACKED, EPI_RESID_XH_SK, g4, chunks, s)) return 1;
            } else if (launch_gemm(dts, nbg, PRO_PACKED, EPI_RESID_XH, g4, chunks, s)) return 1;
        } else if (launch_gemm(dt, nbg, PRO_PACKED, EPI_RESID, g4, chunks, s)) return 1;
    }
    return 0;
}
// final RMSNorm + heads on the h->B decode rows; `form` = how the last run_layers left them (plain_form after a prompt pass / restart)
// `mixed_text`: the text head of a mixed step (text rows beside code rows) -- the text-mode launch over all rows into the text logits, no hidden rows
static int run_heads(ctts_gpt* h, bool write_hidden, StreamForm form, hipStream_t s, bool mixed_text = false) {
    const int nbg = form.nbg, chunks = (h->B + 16 * nbg - 1) / (16 * nbg);
    const bool text = h->text_mode || mixed_text;
    GemmArgs a = {};
    a.st = h->st; a.R = h->B; a.eps = 1e-6f; a.meta = h->meta_dec;
    a.valu = form.valu;
    const int nv = text ? h->vocab_text_head : h->NVQ * h->V;
    a.W = text ? h->whead_text : h->whead; a.n_row_tiles = (nv + 15) / 16; a.K = h->H; a.x = h->x_dec; a.lnw = h->lnf;
    a.logits = mixed_text ? h->logits_text : h->logits; a.n_valid = nv;
    a.dyn = (write_hidden && !mixed_text) ? h->dyn : nullptr;       // the kernel tests dyn->hidden_out itself
    a.rows = h->finend;
    a.opart = h->dpart; a.np = form.parts ? 4 : 0;
    // the last down projection left the rows as packed fp16 + sums of squares (PRO_XH): no fp32 re-normalisation per block.  The text head is a
    // different launch shape (not measured): it keeps the fp32 prologue
    if (form.xh && !text && h->xh_heads && (!form.split || h->whead_sp != nullptr)) {
        a.xh = h->xh; a.ssq = h->ssq; a.scale_in = h->scale_d;
        if (form.split) a.W = h->whead_sp;
        return launch_gemm(form.split ? 2 : h->cfg.dtype, nbg, PRO_XH, EPI_LOGITS, a, chunks, s);
    }
    return launch_gemm(h->cfg.dtype, nbg, (nbg == 1) ? PRO_NORM_P : PRO_NORM, EPI_LOGITS, a, chunks, s);
}

static int run_sample_phase(ctts_gpt* h, StreamForm form, hipStream_t s) {
    if (!form.logits && run_heads(h, true, form, s)) return 1;      // (the persistent launch that ended the stack wrote the logits and the hidden rows itself)
    // Mixed step (a row of the batch is a text row, host mirror text_live): the code heads ran over ALL rows as in any step -- as a launch of their own: the persistent
    // launch drops its fused heads in mixed steps (plan_layers), a text row's code logits are simply not read -- then the text head over all rows into the text logits,
    // the code sampler (its text rows' blocks return) and the text sampler on the text block (its code rows' blocks return).  Every row takes its ticket once, in the kernel of its mode; the last
    // arriver, whichever kernel it runs in, advances the step state.  Both samplers read x_dec-independent inputs (logits, row records) and each writes only its
    // own rows' x_dec / meta / RoPE rows, so the text head must read x_dec BEFORE either of them runs: it is launched first.
    const bool mixed = !h->text_mode && h->text_live > 0;
    if (mixed) {
        if (!h->text_rows_on || !h->dyn_text || !h->logits_text) {
            ctts_set_error("sample / decode: a row of the batch is a text row (mode 1) but ctts_gpt_enable_text_rows has not been called for this generate state");
            return 1;
        }
        StreamForm tf = form;
        tf.logits = false;
        if (run_heads(h, false, tf, s, true)) return 1;
    }
    SamplerArgs sa = {};
    sa.dyn = h->dyn; sa.logits = h->logits; sa.V = h->text_mode ? h->vocab_text_head : h->V; sa.B = h->B; sa.st = h->st;
    sa.text_mode = h->text_mode; sa.mixed = mixed ? 1 : 0;
    sa.emb_code = h->text_mode ? h->emb_text : h->emb_code; sa.H = h->H; sa.x_next = h->x_dec; sa.meta = h->meta_dec; sa.rope = h->rope; sa.rope_rows = h->rope_dec;
    sa.hist_ring = h->hist_ring; sa.finend = h->finend;
    sa.guided = h->guide_on;                     // (read by the text sampler's launch only)
    if (launch_sampler(sa, h->B, s)) return 1;
    if (!mixed) return 0;
    sa.dyn = h->dyn_text; sa.logits = h->logits_text; sa.V = h->vocab_text_head; sa.text_mode = 1; sa.emb_code = h->emb_text;
    return launch_sampler(sa, h->B, s);
}

static int reset_state(ctts_gpt* h, bool keep_draw, hipStream_t s) {
    // step/all_done/ticket <- 0; decode rows back to (slot T-1, pos cum-1); finish/end_idx <- 0
    h->launched = 0;
    CTTS_HIP_CHECK(hipMemsetAsync(&h->st->step, 0, 4, s));
    if (!keep_draw) CTTS_HIP_CHECK(hipMemsetAsync(&h->st->draw, 0, 4, s));
    CTTS_HIP_CHECK(hipMemsetAsync(&h->st->all_done, 0, 8, s));          // all_done + ticket
    CTTS_HIP_CHECK(hipMemcpyAsync(h->meta_dec, h->meta_dec0, h->B * sizeof(RowMeta), hipMemcpyDeviceToDevice, s));
    CTTS_HIP_CHECK(hipMemsetAsync(h->io.finish, 0, h->B * 4, s));
    CTTS_HIP_CHECK(hipMemsetAsync(h->io.end_idx, 0, h->B * 4, s));
    if (!keep_draw) {       // begin: {fin 0, end 0, attempt 0, limit, utterance id} per row (pageable source: staged before the call returns)
        CTTS_HIP_CHECK(hipMemcpyAsync(h->finend, h->finend_host.data(), h->B * sizeof(RowState), hipMemcpyHostToDevice, s));
    } else {
        if (launch_restart_rows(h->finend, h->B, h->guide_on ? h->guide_tab : nullptr, s)) return 1;
        for (HostRow& r : h->rows) r.ctx = h->T;
    }      // ensure_non_empty regenerate: rows that ended at step 0 move on to their next noise attempt
    CTTS_HIP_CHECK(hipMemsetAsync(h->hist_ring, 0xFF, (size_t)h->B * CTTS_NUM_VQ * 16 * 4, s));      // -1: no id sampled yet
    return 0;
}

// per-utterance adapters of sequences 0..B-1 for a call that starts a prompt pass (begin, score): the call starts from what ctts_gpt_set_row_adapters requested.
// (lora_rows is the LIVE state: ctts_gpt_compact clears it once every adapter-carrying row has left the batch and ctts_gpt_admit_adapters rewrites the tables --
// a second generate() after ONE set_row_adapters() call used to run without its adapters, silently)  begin has its rows by now, row b on lane b; score seats none
static int seat_row_adapters(ctts_gpt* h, int B, const char* who, hipStream_t s) {
    if (h->lora_slot_host.empty()) return 0;
    if (h->req.slots.empty()) h->lora_slot_host.assign(CTTS_MAX_B, -1);
    else h->lora_slot_host = h->req.slots;
    for (HostRow& r : h->rows) r.slot = h->lora_slot_host[r.seq];
    const bool failed = lora_summary(h, B, [h](int b) { return h->lora_slot_host[b]; }) != 0;      // (of the sequences: the same as of begin's rows)
    if (failed || (h->lora_rows && h->batch_inv)) {
        if (!failed) ctts_set_error("%s: per-utterance adapters (ctts_gpt_set_row_adapters) are outside the %s contract; set the option to 0 or merge the adapter", who, inv_name(h));
        h->rows.clear(); h->lora_rows = 0; h->lora_mlp = 0; h->B = 0;
        return 1;
    }
    if (h->lora_slot_of_seq)        // (pageable source: staged before the call returns)
        CTTS_HIP_CHECK(hipMemcpyAsync(h->lora_slot_of_seq, h->lora_slot_host.data(), CTTS_MAX_B * 4, hipMemcpyHostToDevice, s));
    // the folded launches tag their granules with the sampler's draw counter, which restarts at every begin(): forget the previous call's granules, or a tile could
    // accept a stale term whose tag happens to match (a previous call of exactly as many steps)
    if (h->lora_rows && h->lora_g) CTTS_HIP_CHECK(hipMemsetAsync(h->lora_g, 0, (size_t)CTTS_MAX_B * 4 * h->H * 8, s));
    return 0;
}

// Shared prompt passes: sequences that name one prompt run it through the prompt pass once, in the lane of the first of them; kv_share.hip hands the others a copy.
extern "C" int ctts_gpt_share_prompts(ctts_gpt* h, int n, const int32_t* prompt_of, int n_prompts) {
    if (!h) { ctts_set_error("share_prompts: null handle"); return 1; }
    h->next.share.clear(); h->next.share_P = 0;      // every call drops the pending table first, a refused one (n < 0 included) too
    if (!prompt_of || n == 0) return 0;
    if (n < 1 || n > h->cfg.max_batch || n_prompts < 1 || n_prompts > n) {
        ctts_set_error("share_prompts: n=%d sequences (max_batch %d) on n_prompts=%d prompts: need 1 <= n_prompts <= n <= max_batch", n, h->cfg.max_batch, n_prompts);
        return 1;
    }
    std::vector<char> named(n_prompts, 0);
    for (int i = 0; i < n; ++i) {
        if (prompt_of[i] < 0 || prompt_of[i] >= n_prompts) { ctts_set_error("share_prompts: prompt_of[%d]=%d outside 0..%d", i, prompt_of[i], n_prompts - 1); return 1; }
        named[prompt_of[i]] = 1;
    }
    for (int p = 0; p < n_prompts; ++p) if (!named[p]) { ctts_set_error("share_prompts: prompt %d is named by no sequence", p); return 1; }
    if (!h->share_dev && dev_alloc(h, (void**)&h->share_dev, (size_t)SH_INTS * 4)) return 1;
    h->next.share.assign(prompt_of, prompt_of + n);
    h->next.share_P = n_prompts;
    return 0;
}
// What share_prompts / admit_sampling / admit_modes named is for the NEXT begin / admit alone, whether it goes through or fails: the call takes it all first, so no later call picks up a stale entry
static NextCall take_next_call(ctts_gpt* h) {
    NextCall taken;
    if (h) std::swap(taken, h->next);
    return taken;
}
// Any generate state ends here: ctts_gpt_begin before it builds the next one, ctts_gpt_score because it overwrites the KV lanes and the prompt workspaces (text_mode, sc, io: begin rewrites them)
static void end_generate_state(ctts_gpt* h) {
    h->B = 0; h->B0 = 0; h->T = 0; h->rows.clear();
    h->admitted = false; h->sampled = false;
    h->segs.clear(); h->pp_rows = 0;  // (debug_read "decode_plan" / "prompt_plan": nothing planned, no prompt pass yet)
    h->share_P = 0; h->share_groups = 0;
    h->text_rows_on = 0;              // every begin switches text rows off again: ctts_gpt_enable_text_rows follows it
    h->guide_on = 0;                  // ... and the guide (begin rewrites the per-call block with a null table): ctts_gpt_set_text_guide follows it
    (void)refresh_rows(h);            // no rows: no text row, no adapter row (nothing to allocate)
}
// the table of one call (kernels.h SH_*): `lanes[i]` = KV lane of the call's i-th sequence.  The prompt pass runs under the leader's adapter slot, so a group shares one slot or none.
static int share_plan(ctts_gpt* h, const std::vector<int>& prompt_of, int P, const int* lanes, const char* who, hipStream_t s) {
    const int n = (int)prompt_of.size();
    std::vector<int>& t = h->share_tab;
    t.assign(SH_INTS, 0);
    for (int p = 0; p < P; ++p) t[SH_LEADER + p] = -1;
    for (int i = 0; i < n; ++i) {
        const int p = prompt_of[i];
        t[SH_PROMPT + i] = p;
        if (t[SH_LEADER + p] < 0) t[SH_LEADER + p] = i;
        const int ld = t[SH_LEADER + p];
        t[SH_LEAD_OF + i] = ld;
        if (!h->lora_slot_host.empty() && h->lora_slot_host[lanes[i]] != h->lora_slot_host[lanes[ld]]) {
            ctts_set_error("%s: sequences %d and %d share prompt %d (ctts_gpt_share_prompts) but carry different adapter slots (%d, %d); the prompt pass depends on the adapter: "
                           "a group shares one slot or none", who, ld, i, p, h->lora_slot_host[lanes[ld]], h->lora_slot_host[lanes[i]]);
            return 1;
        }
    }
    int G = 0, nf = 0;
    for (int p = 0; p < P; ++p) {
        const int ld = t[SH_LEADER + p], first = nf;
        for (int i = 0; i < n; ++i) if (prompt_of[i] == p && i != ld) t[SH_FOLLOWERS + nf++] = lanes[i];
        if (nf == first) continue;
        t[SH_GROUPS + 3 * G] = lanes[ld]; t[SH_GROUPS + 3 * G + 1] = first; t[SH_GROUPS + 3 * G + 2] = nf - first;
        ++G;
    }
    h->share_groups = G;
    CTTS_HIP_CHECK(hipMemcpyAsync(h->share_dev, t.data(), (size_t)SH_INTS * 4, hipMemcpyHostToDevice, s));      // pageable source: staged before the call returns
    return 0;
}
// the leaders' prompt span [0, span) of the cache -> their followers' lanes, after the last prompt pass of the call, in stream order
static int share_kv(ctts_gpt* h, int span, hipStream_t s) {
    if (h->share_groups == 0 || span <= 0) return 0;
    KvShareArgs a = {};
    a.kv = h->kv; a.run_bytes = (size_t)h->cfg.max_seq * CTTS_HEAD_DIM * h->esz; a.lane_bytes = a.run_bytes * h->NH; a.plane_bytes = a.lane_bytes * h->cfg.max_batch;
    a.groups = h->share_dev + SH_GROUPS; a.followers = h->share_dev + SH_FOLLOWERS; a.n_groups = h->share_groups; a.NH = h->NH;
    a.units = (unsigned)((size_t)span * CTTS_HEAD_DIM * h->esz / 16);
    return launch_kv_share(a, h->L * 2 * h->NH, s);
}

// ctts_gpt_begin with the requests it took.  The share table is spent whatever happens.  The admission requests (req.modes, req.knobs) are cleared HERE, at the point
// from which the call has dropped them even if it fails further down; what a failed call leaves in `req` goes back to the handle (ctts_gpt_begin).
static int begin_state(ctts_gpt* h, int B, int T, const int32_t* mask, const ctts_sampler_cfg* sc, const ctts_gen_io* io, void* stream, NextCall& req) {
    const std::vector<int>& share = req.share; const int share_P = req.share_P;
    if (!h || !h->finalized || !h->kv || !h->rope) { ctts_set_error("begin: handle not ready (finalize / bind_kv / set_rope)"); return 1; }
    if (!mask || !sc || !io || !io->ids || !io->finish || !io->end_idx) { ctts_set_error("begin: null argument"); return 1; }
    CTTS_RANGE("ctts_gpt_begin");               // reference: nvtx "adjust_buffer" / "set_tensors" (trt_models/predictor.py:142,159)
    if (B < 1 || B > h->cfg.max_batch || T < 1 || T + sc->max_new_token > h->cfg.max_seq) {
        ctts_set_error("begin: B=%d T=%d max_new=%d exceed max_batch=%d / max_seq=%d", B, T, sc->max_new_token, h->cfg.max_batch, h->cfg.max_seq);
        return 1;
    }
    if (!share.empty()) {
        if ((int)share.size() != B) { ctts_set_error("begin: ctts_gpt_share_prompts named the prompts of %d sequences, this call has B=%d", (int)share.size(), B); return 1; }
        if (sc->infer_text) { ctts_set_error("begin: shared prompt passes (ctts_gpt_share_prompts) are code mode only; the refine-text pass (infer_text) runs every prompt"); return 1; }
    }
    // row modes of this call (ctts_gpt_set_row_modes): checked before anything changes
    bool any_text = false;
    for (int b = 0; b < B && b < (int)h->req.modes.size(); ++b) any_text = any_text || h->req.modes[b] == 1;
    if (any_text) {
        if (sc->infer_text) { ctts_set_error("begin: text rows (ctts_gpt_set_row_modes) live in a code-mode call; this call's own infer_text is 1 -- every row of it is a text row already"); return 1; }
        if (!h->whead_text || !h->emb_text) { ctts_set_error("begin: a text row (ctts_gpt_set_row_modes) needs head_text.* and emb_text.weight"); return 1; }
        if (io->noise != nullptr) { ctts_set_error("begin: text rows (ctts_gpt_set_row_modes) need device noise (caller-supplied noise is laid out for one mode's rows)"); return 1; }
        if (!share.empty()) { ctts_set_error("begin: shared prompt passes (ctts_gpt_share_prompts) are for code rows; this call seats a text row (ctts_gpt_set_row_modes)"); return 1; }
        const RowSampling call_knobs = knobs_of_cfg(cfg_of_abi(*sc));      // (set_row_sampling names every sequence: an entry equal to the call's values is no knob of its own)
        for (int b = 0; b < B && b < (int)h->req.knobs.size() && b < (int)h->req.modes.size(); ++b)
            if (h->req.modes[b] == 1 && !same_knobs(h->req.knobs[b], call_knobs)) {
                ctts_set_error("begin: sequence %d is a text row (ctts_gpt_set_row_modes) and carries per-row sampling knobs (ctts_gpt_set_row_sampling); text rows keep the values of ctts_gpt_enable_text_rows", b);
                return 1;
            }
    }
    // From here on the call's mode is written, the text rows are off and the modes named for an admission dropped -- for the previous state too, should a refusal below leave it standing (as always)
    h->text_mode = sc->infer_text ? 1 : 0; h->text_rows_on = 0; h->text_live = 0;
    req.modes.clear();
    if (h->text_mode) {
        if (!h->whead_text || !h->emb_text) { ctts_set_error("begin: infer_text needs head_text.* and emb_text.weight"); return 1; }
        if (sc->use_penalty) { ctts_set_error("begin: infer_text supports repetition_penalty == 1 only (the reference's processor mis-broadcasts the [B,n,1] history in this mode)"); return 1; }
        if (sc->eos_token >= h->vocab_text_head) { ctts_set_error("begin: eos out of range"); return 1; }
    } else if (sc->past_window > 16 || sc->eos_token >= h->V) { ctts_set_error("begin: past_window>16 or eos out of range"); return 1; }
    if (h->batch_inv && h->cfg.dtype == CTTS_DTYPE_F16 && io->noise != nullptr) {
        // (fp32 engines keep accepting it -- the reference goldens replay torch's draws under the option -- though it is outside the contract there too)
        ctts_set_error("begin: caller-supplied noise is indexed by the batch's draw counter and is outside the schedule_invariant contract; use device noise or set the option to 0");
        return 1;
    }
    if (h->batch_inv && h->cfg.dtype == CTTS_DTYPE_F32 && !(h->split_ok && h->wsplit && h->whead_sp)) {
        ctts_set_error("begin: batch_invariant needs the head / tail weight images, and a weight of this checkpoint is beyond the fp16 range (x 64)");
        return 1;
    }
    if (!h->req.knobs.empty()) {       // per-utterance sampling knobs (ctts_gpt_set_row_sampling)
        if (h->text_mode) { ctts_set_error("begin: per-utterance sampling parameters (set_row_sampling) are code mode only; the refine-text pass (infer_text) keeps the call's values"); return 1; }
        for (int b = 0; b < B && b < (int)h->req.knobs.size(); ++b) {
            ctts_row_sampling p;
            memcpy(&p, &h->req.knobs[b], sizeof(p));
            if (check_knobs(p, sc->max_new_token, "begin (set_row_sampling)", b)) return 1;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    end_generate_state(h);
    h->B = B; h->B0 = B; h->T = T; h->io = *io;
    h->finend_host.assign(B, RowState{}); h->seq_host.resize(B);
    for (int b = 0; b < B; ++b) {       // sequence b sits in row b and KV lane b
        RowState& r = h->finend_host[b];
        const unsigned long long uid = io->utt_ids ? io->utt_ids[b] : (unsigned long long)b;
        int lim = io->row_limits ? io->row_limits[b] : sc->max_new_token;
        r.limit = lim < 1 ? 1 : (lim > sc->max_new_token ? sc->max_new_token : lim);
        r.uid_lo = (unsigned)uid; r.uid_hi = (unsigned)(uid >> 32);
        r.out = b;
        r.mode = (any_text && b < (int)h->req.modes.size() && h->req.modes[b] == 1) ? 1 : 0;
        h->rows.push_back(HostRow{b, T, T + r.limit, r.mode, -1});
        h->seq_host[b] = b;
    }
    if (refresh_rows(h) || seat_row_adapters(h, B, "begin", s)) return 1;
    if (!share.empty()) {
        if (share_plan(h, share, share_P, h->seq_host.data(), "begin", s)) { h->B = 0; h->rows.clear(); return 1; }
        h->share_P = share_P;
    }
    const int* share_dev = h->share_P ? h->share_dev : nullptr;
    h->io.utt_ids = nullptr; h->io.row_limits = nullptr;      // host arrays are consumed here, not kept
    h->sc = cfg_of_abi(*sc);
    SamplerDyn d = {};
    d.cfg = h->sc; d.n_draws = io->n_draws; d.ids = io->ids; d.finish = io->finish; d.end_idx = io->end_idx; d.noise = io->noise;
    d.seed = io->seed; d.hidden_out = io->hiddens; d.hidden_stride = sc->max_new_token * h->H;
    d.rows0 = B * (h->text_mode ? 1 : CTTS_NUM_VQ);
    CTTS_HIP_CHECK(hipMemcpyAsync(h->dyn, &d, sizeof(d), hipMemcpyHostToDevice, s));       // pageable source: staged before the call returns
    // the rows' sampling knobs: the call's values, then what set_row_sampling requested per sequence
    h->knobs_host.assign(B, knobs_of_cfg(h->sc));
    for (int b = 0; b < B && b < (int)h->req.knobs.size(); ++b) h->knobs_host[b] = h->req.knobs[b];
    req.knobs.clear();               // the new rows have their knobs: what was named for an admission into the previous state is dropped
    CTTS_HIP_CHECK(hipMemcpyAsync(h->knobs, h->knobs_host.data(), (size_t)B * sizeof(RowSampling), hipMemcpyHostToDevice, s));
    if (launch_fill_meta(h->meta_pre, h->meta_dec0, h->st, mask, B, T, h->rope, h->rope_pre, share_dev, h->share_P ? h->share_P : B, s)) return 1;
    if (h->batch_inv) {
        // the prompt is laid out like an admission of every row (ctts_gpt_admit): T - 1 prompt rows per sequence for the prompt pass, the decode rows at the last
        // token (slot T - 1: the same RowMeta as meta_dec0) with its RoPE row -- ctts_gpt_prefill fills x_dec with the last tokens' embeddings
        CTTS_HIP_CHECK(hipMemcpyAsync(h->keep_dev, h->seq_host.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));      // rows == KV lanes
        CTTS_HIP_CHECK(hipMemcpyAsync(h->cfin, h->finend_host.data(), (size_t)B * sizeof(RowState), hipMemcpyHostToDevice, s));
        AdmitArgs a = {};
        a.mask = mask; a.emb = nullptr; a.rows = h->keep_dev; a.seqs = h->keep_dev; a.fresh = h->cfin; a.n = B; a.T = T; a.H = h->H;
        a.pm = h->meta_pre; a.rope_pre = h->rope_pre; a.dm = h->meta_dec; a.rope_dec = h->rope_dec; a.x_dec = h->x_dec; a.ring = h->hist_ring; a.finend = h->finend;
        a.rope = h->rope; a.st = h->st; a.finish = io->finish; a.end_idx = io->end_idx; a.begin = 1; a.share = share_dev;
        if (launch_admit_rows(a, s)) return 1;
        CTTS_HIP_CHECK(hipMemcpyAsync(h->rope_dec0, h->rope_dec, (size_t)B * 64 * 4, hipMemcpyDeviceToDevice, s));
    }
    CTTS_HIP_CHECK(hipMemsetAsync(h->sat, 0, 4, s));
    if (h->pl_error) CTTS_HIP_CHECK(hipMemsetAsync(h->pl_error, 0, 4, s));
    return reset_state(h, false, s);
}
extern "C" int ctts_gpt_begin(ctts_gpt* h, int B, int T, const int32_t* mask, const ctts_sampler_cfg* sc, const ctts_gen_io* io, void* stream) {
    NextCall req = take_next_call(h);
    const int rc = begin_state(h, B, T, mask, sc, io, stream, req);
    // A refused begin hands back the admission requests it had not dropped yet (begin_state): refused before it touches anything, it leaves the previous generate
    // state standing, and what ctts_gpt_admit_sampling / ctts_gpt_admit_modes named for that state's next admission with it.  The share table never goes back.
    if (rc && h) { h->next.knobs = std::move(req.knobs); h->next.modes = std::move(req.modes); }
    return rc;
}

// The one prompt-pass loop (prefill, the invariant prefill, score, admit): R prompt rows of T_rows tokens per sequence, laid out from meta_pre[0] on, through the layers
// in passes of at most pass_rows rows.  stage(r0, n) fills x_pre[0, n) with rows r0 .. r0 + n - 1, after(r0, n) takes what the layers left there.
template <class Stage, class After>
static int prompt_passes(ctts_gpt* h, long R, int T_rows, hipStream_t s, Stage stage, After after) {
    for (long r0 = 0; r0 < R; r0 += h->pass_rows) {
        const int n = (int)(R - r0 < h->pass_rows ? R - r0 : h->pass_rows);
        if (stage(r0, n) || run_layers(h, h->x_pre, h->meta_pre + r0, h->rope_pre + (size_t)r0 * 64, n, DecodePath{1, 0}, nullptr, s, nullptr, T_rows) || after(r0, n)) return 1;
    }
    return 0;
}
// stage: rows of the caller's [.][T] embeddings as they lie (prefill, score)
static int stage_rows(ctts_gpt* h, const float* emb, long r0, int n, hipStream_t s) {
    CTTS_HIP_CHECK(hipMemcpyAsync(h->x_pre, emb + (size_t)r0 * h->H, (size_t)n * h->H * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}
// stage: rows of the [.][T - 1] layout -- every sequence without its last token -- from [.][T] embeddings (the invariant prefill; ctts_gpt_admit: one pass, one 2-D copy)
static int stage_rows_but_last(ctts_gpt* h, const float* emb, int T, long r0, int n, hipStream_t s) {
    const long Tm = T - 1, H = h->H;
    for (long r = r0; r < r0 + n;) {             // x_pre[0, n) <- prompt rows r0 .. r0 + n - 1
        const long b = r / Tm, t = r % Tm, left = r0 + n - r;
        if (t == 0 && left >= Tm) {
            const long nb = left / Tm;
            CTTS_HIP_CHECK(hipMemcpy2DAsync(h->x_pre + (size_t)(r - r0) * H, (size_t)Tm * H * 4, emb + (size_t)b * T * H, (size_t)T * H * 4, (size_t)Tm * H * 4, nb,
                                            hipMemcpyDeviceToDevice, s));
            r += nb * Tm;
        } else {
            const long len = (Tm - t < left) ? Tm - t : left;
            CTTS_HIP_CHECK(hipMemcpyAsync(h->x_pre + (size_t)(r - r0) * H, emb + ((size_t)b * T + t) * H, (size_t)len * H * 4, hipMemcpyDeviceToDevice, s));
            r += len;
        }
    }
    return 0;
}
static int no_after(long, int) { return 0; }

// batch_invariant prompt pass: the first T - 1 tokens of every sequence, laid out [B][T - 1] (ctts_gpt_begin), in passes of at most pass_rows rows; the last
// token's embedding becomes the decode row's input, which ctts_gpt_sample runs through the first layer pass -- the admission path (ctts_gpt_admit), so a begun
// utterance and an admitted one take the same arithmetic.  Shared prompt passes: emb and the layout are per PROMPT ([P][T - 1] rows in the leaders' lanes); every
// sequence takes its prompt's last embedding, the followers a copy of the span [0, T - 1)
static int prefill_invariant(ctts_gpt* h, const float* emb, hipStream_t s) {
    const int B = h->B, T = h->T, Tm = T - 1, H = h->H, P = h->share_P ? h->share_P : B;
    const long R = (long)P * Tm;
    h->pp_rows = R; h->pp_T = Tm;
    if (prompt_passes(h, R, Tm, s, [&](long r0, int n) { return stage_rows_but_last(h, emb, T, r0, n, s); }, no_after)) return 1;
    if (h->share_P) {
        if (launch_share_rows(emb + (size_t)Tm * H, (size_t)T * H, h->share_dev + SH_PROMPT, h->x_dec, B, H, s) || share_kv(h, Tm, s)) return 1;
    } else
        CTTS_HIP_CHECK(hipMemcpy2DAsync(h->x_dec, (size_t)H * 4, emb + (size_t)Tm * H, (size_t)T * H * 4, (size_t)H * 4, B, hipMemcpyDeviceToDevice, s));
    CTTS_HIP_CHECK(hipMemcpyAsync(h->x_last, h->x_dec, (size_t)B * H * 4, hipMemcpyDeviceToDevice, s));       // (ensure_non_empty restarts replay from here)
    return 0;
}

extern "C" int ctts_gpt_prefill(ctts_gpt* h, const float* emb, void* stream) {
    if (!h || !emb || h->B == 0) { ctts_set_error("prefill: call begin first"); return 1; }
    CTTS_RANGE("ctts_gpt_prefill");             // reference: nvtx "forward" (trt_models/llama_trt_model.py:44,74), q_len > 1
    hipStream_t s = (hipStream_t)stream;
    if (h->batch_inv) return prefill_invariant(h, emb, s);
    // shared prompt passes: P prompts in the leaders' lanes; their last residual rows land in the leaders' decode rows, the followers get a copy of both
    const int P = h->share_P ? h->share_P : h->B;
    const long R = (long)P * h->T;
    h->pp_rows = R; h->pp_T = h->T;
    // after a pass: rows (b, T-1) that live in it -> x_dec[b]  (indices computed on the device: the call stays asynchronous)
    if (prompt_passes(h, R, h->T, s, [&](long r0, int n) { return stage_rows(h, emb, r0, n, s); }, [&](long r0, int n) {
            return launch_gather_last_rows(h->x_pre, h->x_dec, P, h->T, (int)r0, n, h->H, h->share_P ? h->share_dev + SH_LEADER : nullptr, s); })) return 1;
    if (h->share_P && (launch_share_rows(h->x_dec, (size_t)h->H, h->share_dev + SH_LEAD_OF, h->x_dec, h->B, h->H, s) || share_kv(h, h->T, s))) return 1;
    // keep a copy of the prompt's last residual rows for ensure_non_empty restarts
    CTTS_HIP_CHECK(hipMemcpyAsync(h->x_last, h->x_dec, (size_t)h->B * h->H * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

// Teacher-forced scoring (include/ctts_hip.h ctts_gpt_score, ctts_gpt_score_text): one path, two heads.  The prompt pass of ctts_gpt_prefill over [B][T], then per
// pass the scored rows (the last n_b of sequence b) are gathered `chunk` at a time, the final RMSNorm + the head run on them (the decode heads' launch, PRO_NORM /
// EPI_LOGITS: every row index it forms is size_t, bounded by R, and it reads no decode state -- st, dyn, rows null) and score.hip reduces the logits.
struct ScoreHead {
    const char* name;                            // "score" / "score_text": the prefix of every message; "ctts_gpt_" + name is the profiler range
    const void* W;                               // head weights
    int NV, V;                                   // logits width; the vocabulary a target indexes (one codebook of the four / the whole text row)
    int cols;                                    // results per target: logprob / argmax are [B][max_targets][cols]
    int chunk;                                   // rows per heads launch: bounds the scratch
    ctts_gpt::ScoreScratch* scratch;
    int (*reduce)(const float* logits, const int* oidx, const int* targets, float* logprob, int* argmax, int m, int V, int n_valid, hipStream_t s);
};
static bool score_ready(const ctts_gpt* h, const char* name) {
    if (h && h->finalized && h->kv && h->rope) return true;
    ctts_set_error("%s: handle not ready (finalize / bind_kv / set_rope)", name);
    return false;
}
static int score_rows(ctts_gpt* h, const ScoreHead& hd, int B, int T, const int32_t* mask, const float* emb, const int32_t* targets, const int32_t* n_targets, int max_targets,
                      float* logprob, int32_t* argmax, hipStream_t s) {
    if (!mask || !emb || !targets || !n_targets || !logprob || !argmax) { ctts_set_error("%s: null argument", hd.name); return 1; }
    if (B < 1 || B > h->cfg.max_batch) { ctts_set_error("%s: B=%d outside 1..max_batch=%d", hd.name, B, h->cfg.max_batch); return 1; }
    if (T < 1 || T > h->cfg.max_seq) { ctts_set_error("%s: T=%d outside 1..max_seq=%d", hd.name, T, h->cfg.max_seq); return 1; }
    if (max_targets < 1) { ctts_set_error("%s: max_targets=%d < 1", hd.name, max_targets); return 1; }
    for (int b = 0; b < B; ++b) {
        const int nb = n_targets[b];
        if (nb < 1 || nb > T || nb > max_targets) {
            ctts_set_error("%s: n_targets[%d]=%d outside 1..min(T=%d, max_targets=%d)", hd.name, b, nb, T, max_targets);
            return 1;
        }
    }
    if (h->batch_inv && h->cfg.dtype == CTTS_DTYPE_F32 && !(h->split_ok && h->wsplit)) {
        ctts_set_error("%s: batch_invariant needs the head / tail weight images, and a weight of this checkpoint is beyond the fp16 range (x 64)", hd.name);
        return 1;
    }
    CTTS_RANGE((std::string("ctts_gpt_") + hd.name).c_str());
    end_generate_state(h);            // the KV lanes and the prompt workspaces are overwritten
    h->text_mode = 0;
    if (seat_row_adapters(h, B, hd.name, s)) return 1;
    ctts_gpt::ScoreScratch& sc = *hd.scratch;
    if (sc.oidx == nullptr) {
        if (!sc.x && dev_alloc(h, (void**)&sc.x, (size_t)hd.chunk * h->H * 4)) return 1;
        if (!sc.logits && dev_alloc(h, (void**)&sc.logits, (size_t)hd.chunk * hd.NV * 4)) return 1;
        if (dev_alloc(h, (void**)&sc.oidx, (size_t)hd.chunk * 4)) return 1;
    }
    // entries j >= n_b: logprob 0, argmax -1
    CTTS_HIP_CHECK(hipMemsetAsync(logprob, 0, (size_t)B * max_targets * hd.cols * 4, s));
    CTTS_HIP_CHECK(hipMemsetAsync(argmax, 0xFF, (size_t)B * max_targets * hd.cols * 4, s));
    if (launch_fill_meta(h->meta_pre, h->meta_dec0, h->st, mask, B, T, h->rope, h->rope_pre, nullptr, B, s)) return 1;
    const long R = (long)B * T;
    h->pp_rows = R; h->pp_T = T;
    // batch_invariant: the heads on 16-row chunks whatever the block holds (as run_heads pins nbg = 1); the chunk only bounds the scratch
    const int nbg = h->batch_inv ? 1 : 2;
    ScoreRows sr = {};
    sr.B = B; sr.max_targets = max_targets;
    return prompt_passes(h, R, T, s, [&](long r0, int n) { return stage_rows(h, emb, r0, n, s); }, [&](long r0, int n) {
        // the scored rows of this pass: sequence b's rows [b T + T - n_b, b T + T) clipped to [r0, r0 + n)
        sr.cum[0] = 0;
        for (int b = 0; b < B; ++b) {
            const long s0 = (long)b * T + T - n_targets[b], s1 = (long)b * T + T;
            const long lo = s0 > r0 ? s0 : r0, hi = s1 < r0 + n ? s1 : r0 + n;
            const int cnt = hi > lo ? (int)(hi - lo) : 0;
            sr.first[b] = cnt ? (int)(lo - r0) : 0;
            sr.j0[b] = cnt ? (int)(lo - s0) : 0;
            sr.cum[b + 1] = sr.cum[b] + cnt;
        }
        for (int g0 = 0; g0 < sr.cum[B]; g0 += hd.chunk) {
            const int m = sr.cum[B] - g0 < hd.chunk ? sr.cum[B] - g0 : hd.chunk;
            if (launch_score_gather(h->x_pre, sc.x, sc.oidx, g0, m, sr, s)) return 1;
            GemmArgs a = {};
            a.R = m; a.eps = 1e-6f; a.W = hd.W; a.n_row_tiles = (hd.NV + 15) / 16; a.K = h->H; a.x = sc.x; a.lnw = h->lnf;
            a.logits = sc.logits; a.n_valid = hd.NV;
            if (launch_gemm(h->cfg.dtype, nbg, PRO_NORM, EPI_LOGITS, a, (m + 16 * nbg - 1) / (16 * nbg), s)) return 1;
            if (hd.reduce(sc.logits, sc.oidx, targets, logprob, argmax, m, hd.V, hd.NV, s)) return 1;
        }
        return 0;
    });
}
// the code heads: SCORE_ROWS rows per launch, four codebooks of V in one 4 * V wide row
extern "C" int ctts_gpt_score(ctts_gpt* h, int B, int T, const int32_t* mask, const float* emb, const int32_t* targets, const int32_t* n_targets, int max_targets,
                              float* logprob, int32_t* argmax, void* stream) {
    if (!score_ready(h, "score")) return 1;
    const ScoreHead hd = {"score", h->whead, h->NVQ * h->V, h->V, CTTS_NUM_VQ, SCORE_ROWS, &h->score_code, launch_score_reduce};
    return score_rows(h, hd, B, T, mask, emb, targets, n_targets, max_targets, logprob, argmax, (hipStream_t)stream);
}
// the refine-text head: the text-head launch of a decode step (run_heads' text shape) on at most max_batch rows at a time, score.hip's one-row-per-workgroup reduce
static int reduce_text(const float* logits, const int* oidx, const int* targets, float* logprob, int* argmax, int m, int V, int, hipStream_t s) {
    return launch_score_text_reduce(logits, oidx, targets, logprob, argmax, m, V, s);
}
extern "C" int ctts_gpt_score_text(ctts_gpt* h, int B, int T, const int32_t* mask, const float* emb, const int32_t* targets, const int32_t* n_targets, int max_targets,
                                   float* logprob, int32_t* argmax, void* stream) {
    if (!score_ready(h, "score_text")) return 1;
    if (!h->whead_text || !h->emb_text) { ctts_set_error("score_text: the engine has no text head (head_text.* and emb_text.weight are needed)"); return 1; }
    const ScoreHead hd = {"score_text", h->whead_text, h->vocab_text_head, h->vocab_text_head, 1, h->score_text_chunk, &h->score_text, reduce_text};
    return score_rows(h, hd, B, T, mask, emb, targets, n_targets, max_targets, logprob, argmax, (hipStream_t)stream);
}

static int run_decode_step(ctts_gpt* h, DecodePath path, hipStream_t s);
static inline DecodePath pick_decode_path(const ctts_gpt* h, int longest);

// Log-probs of the sampled ids (include/ctts_hip.h): the two destinations are the last words of the per-call block the sampler reads (SamplerDyn), so a
// captured decode graph serves calls with and without them; begin's rewrite of the block leaves both null.
extern "C" int ctts_gpt_set_logprob_out(ctts_gpt* h, float* lp_raw, float* lp_sampled, void* stream) {
    if (!h || h->B == 0) { ctts_set_error("set_logprob_out: no generate state (call ctts_gpt_begin first)"); return 1; }
    if (h->text_mode) { ctts_set_error("set_logprob_out: the refine-text pass (infer_text) returns no log-probs; code mode only"); return 1; }
    if (h->sampled) { ctts_set_error("set_logprob_out: called after the first ctts_gpt_sample / ctts_gpt_decode of this call; set the buffers right after ctts_gpt_begin"); return 1; }
    float* const p[2] = {lp_raw, lp_sampled};
    static_assert(offsetof(SamplerDyn, lp_sampled) == offsetof(SamplerDyn, lp_raw) + sizeof(float*), "the two destinations are copied as one pair");
    CTTS_HIP_CHECK(hipMemcpyAsync((char*)h->dyn + offsetof(SamplerDyn, lp_raw), p, sizeof(p), hipMemcpyHostToDevice, (hipStream_t)stream));      // pageable source: staged before the call returns
    return 0;
}

// Log-probs of the text rows' sampled ids (include/ctts_hip.h): the same two words of the block the TEXT sampler reads -- the call's own block of an infer_text
// call (where the code entry point above refuses), the text block of a code call with text rows (which the code sampler never reads).  begin and
// ctts_gpt_enable_text_rows rewrite their block whole: both destinations are null again.
extern "C" int ctts_gpt_set_text_logprob_out(ctts_gpt* h, float* lp_raw, float* lp_sampled, void* stream) {
    if (!h || h->B == 0) { ctts_set_error("set_text_logprob_out: no generate state (call ctts_gpt_begin first)"); return 1; }
    if (!h->text_mode && !h->text_rows_on) { ctts_set_error("set_text_logprob_out: a code call without text rows: the call must be an infer_text call, or ctts_gpt_enable_text_rows must come first"); return 1; }
    if (h->sampled) { ctts_set_error("set_text_logprob_out: called after the first ctts_gpt_sample / ctts_gpt_decode of this call; set the buffers right after ctts_gpt_begin / ctts_gpt_enable_text_rows"); return 1; }
    float* const p[2] = {lp_raw, lp_sampled};
    SamplerDyn* const blk = h->text_mode ? h->dyn : h->dyn_text;
    CTTS_HIP_CHECK(hipMemcpyAsync((char*)blk + offsetof(SamplerDyn, lp_raw), p, sizeof(p), hipMemcpyHostToDevice, (hipStream_t)stream));      // pageable source: staged before the call returns
    return 0;
}

// ---- text rows beside code rows (include/ctts_hip.h; RowState.mode) --------------------------------------------------------------------------------------------
extern "C" int ctts_gpt_set_row_modes(ctts_gpt* h, const int32_t* modes, int B) {
    if (!h) { ctts_set_error("set_row_modes: null handle"); return 1; }
    if (!modes || B <= 0) { h->req.modes.clear(); return 0; }
    if (B > CTTS_MAX_B) { ctts_set_error("set_row_modes: B=%d > %d", B, CTTS_MAX_B); return 1; }
    for (int b = 0; b < B; ++b) if (modes[b] != 0 && modes[b] != 1) { ctts_set_error("set_row_modes: sequence %d: mode %d (0 = code, 1 = text)", b, modes[b]); return 1; }
    h->req.modes.assign(modes, modes + B);
    return 0;
}
extern "C" int ctts_gpt_admit_modes(ctts_gpt* h, int n, const int32_t* rows, const int32_t* modes, void* stream) {
    (void)stream;        // host-side request: the next ctts_gpt_admit seats the modes
    if (!h || h->B == 0 || !rows || !modes || n < 0) { ctts_set_error("admit_modes: call begin first / null argument"); return 1; }
    bool any = false;
    if (check_rows(h, "admit_modes", n, rows, false, [&](int i) {
            if (modes[i] != 0 && modes[i] != 1) { ctts_set_error("admit_modes: entry %d: mode %d (0 = code, 1 = text)", i, modes[i]); return 1; }
            any = any || modes[i] == 1;
            return 0;
        })) return 1;
    if (any && h->text_mode) { ctts_set_error("admit_modes: this call's own infer_text is 1: every row of it is a text row already; text rows beside code rows live in a code-mode call"); return 1; }
    if (any && !h->text_rows_on) { ctts_set_error("admit_modes: a mode-1 row needs ctts_gpt_enable_text_rows first (after ctts_gpt_begin, before the row is seated)"); return 1; }
    for (int i = 0; i < n; ++i) name_row(h->next.modes, rows[i], (int)modes[i]);
    return 0;
}
extern "C" int ctts_gpt_enable_text_rows(ctts_gpt* h, const ctts_sampler_cfg* tsc, int32_t* text_ids_dev, void* stream) {
    if (!h || h->B == 0) { ctts_set_error("enable_text_rows: no generate state (call ctts_gpt_begin first)"); return 1; }
    if (!tsc || !text_ids_dev) { ctts_set_error("enable_text_rows: null argument"); return 1; }
    if (h->text_mode) { ctts_set_error("enable_text_rows: this call's own infer_text is 1: every row of it is a text row already; text rows beside code rows live in a code-mode call"); return 1; }
    if (!tsc->infer_text) { ctts_set_error("enable_text_rows: text_sc must be the refine-text pass's parameters (infer_text = 1)"); return 1; }
    if (!h->whead_text || !h->emb_text) { ctts_set_error("enable_text_rows: text rows need head_text.* and emb_text.weight"); return 1; }
    if (tsc->use_penalty) { ctts_set_error("enable_text_rows: text rows support repetition_penalty == 1 only (use_penalty must be 0, as for infer_text)"); return 1; }
    if (h->io.noise != nullptr) { ctts_set_error("enable_text_rows: device noise only (caller-supplied noise is laid out for one mode's rows)"); return 1; }
    if (tsc->eos_token < 0 || tsc->eos_token >= h->vocab_text_head) { ctts_set_error("enable_text_rows: eos out of range"); return 1; }
    if (!std::isfinite(tsc->temperature[0]) || !(tsc->temperature[0] > 0.f)) { ctts_set_error("enable_text_rows: temperature[0] = %g (must be finite and > 0)", (double)tsc->temperature[0]); return 1; }
    if (tsc->max_new_token < 1 || tsc->max_new_token > h->sc.max_new) {
        // the stores keyed by the row's output slot and its own step that are not the samplers' (the heads' hidden rows [slot][step < max_new_token]) stay inside the
        // utterance's own slot only while a text row's step stays below the code call's max_new_token
        ctts_set_error("enable_text_rows: the text rows' max_new_token = %d must be 1..%d, the code call's max_new_token (a text row's step indexes the call's per-slot arrays)", tsc->max_new_token, h->sc.max_new);
        return 1;
    }
    if (tsc->min_new_token > tsc->max_new_token) { ctts_set_error("enable_text_rows: min_new_token = %d > max_new_token = %d", tsc->min_new_token, tsc->max_new_token); return 1; }
    if (h->sampled && h->text_live > 0) { ctts_set_error("enable_text_rows: a text row seated by ctts_gpt_begin needs the call before the first ctts_gpt_sample / ctts_gpt_decode"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    if (!h->dyn_text && dev_alloc(h, (void**)&h->dyn_text, sizeof(SamplerDyn))) return 1;
    if (!h->logits_text && dev_alloc(h, (void**)&h->logits_text, (size_t)CTTS_MAX_B * h->vocab_text_head * 4)) return 1;
    h->sc_text = cfg_of_abi(*tsc);
    SamplerDyn d = {};
    d.cfg = h->sc_text; d.n_draws = 1; d.ids = text_ids_dev; d.finish = h->io.finish; d.end_idx = h->io.end_idx; d.noise = nullptr;
    d.seed = h->io.seed; d.hidden_out = nullptr; d.hidden_stride = 0; d.rows0 = h->B0;
    CTTS_HIP_CHECK(hipMemcpyAsync(h->dyn_text, &d, sizeof(d), hipMemcpyHostToDevice, s));       // pageable source: staged before the call returns
    // text rows that begin seated (ctts_gpt_set_row_modes): their limit is the text rows' own (begin clamped it to the code call's)
    if (h->text_live > 0) {
        for (int b = 0; b < h->B; ++b)
            if (h->finend_host[b].mode == 1 && h->finend_host[b].limit > h->sc_text.max_new) { h->finend_host[b].limit = h->sc_text.max_new; h->rows[b].cap = h->T + h->sc_text.max_new; }
        CTTS_HIP_CHECK(hipMemcpyAsync(h->finend, h->finend_host.data(), (size_t)h->B * sizeof(RowState), hipMemcpyHostToDevice, s));
    }
    h->text_rows_on = 1;
    h->guide_on = 0;                  // (the block was rewritten with a null table: ctts_gpt_set_text_guide follows this call)
    return 0;
}

// ---- guided refine-text (include/ctts_hip.h; kernels.h GuideTab) -----------------------------------------------------------------------------------------------
#define GUIDE_PIN_INTS 65536      // ints per slot of the pinned upload ring (4 slots; a record is at most 1024 ints)
// The per-call part is checked here for the hook as well: free ids distinct, in range, none the EOS.
static int check_free_ids(const char* who, const int32_t* free_ids, int n_free, int max_run, int eos, int vocab) {
    if (n_free < 0 || n_free > CTTS_GUIDE_MAX_FREE) { ctts_set_error("%s: %d free ids (at most %d)", who, n_free, CTTS_GUIDE_MAX_FREE); return 1; }
    if (n_free > 0 && !free_ids) { ctts_set_error("%s: null free_ids", who); return 1; }
    if (max_run < 0) { ctts_set_error("%s: max_run = %d (must be >= 0)", who, max_run); return 1; }
    for (int i = 0; i < n_free; ++i) {
        if (free_ids[i] < 0 || free_ids[i] >= vocab) { ctts_set_error("%s: free id %d outside 0..%d", who, free_ids[i], vocab - 1); return 1; }
        if (free_ids[i] == eos) { ctts_set_error("%s: free id %d is the EOS token (the guide ends a row by EOS alone)", who, free_ids[i]); return 1; }
        for (int j = 0; j < i; ++j) if (free_ids[j] == free_ids[i]) { ctts_set_error("%s: free id %d is listed twice", who, free_ids[i]); return 1; }
    }
    return 0;
}
static int check_guide_src(const char* who, int i, const int32_t* src, int n, int limit, int eos, int vocab) {
    if (n > CTTS_GUIDE_MAX_SRC) { ctts_set_error("%s: entry %d: source of %d ids (at most %d)", who, i, n, CTTS_GUIDE_MAX_SRC); return 1; }
    if (n + 1 > limit) { ctts_set_error("%s: entry %d: a source of %d ids needs %d tokens (the source and EOS), the row's limit is %d", who, i, n, n + 1, limit); return 1; }
    for (int k = 0; k < n; ++k) {
        if (src[k] < 0 || src[k] >= vocab) { ctts_set_error("%s: entry %d: source id %d outside 0..%d", who, i, src[k], vocab - 1); return 1; }
        if (src[k] == eos) { ctts_set_error("%s: entry %d: source id %d is the EOS token", who, i, src[k]); return 1; }
    }
    return 0;
}

extern "C" int ctts_gpt_set_text_guide(ctts_gpt* h, const int32_t* free_ids, int n_free, int max_run, void* stream) {
    if (!h || h->B == 0) { ctts_set_error("set_text_guide: no generate state (call ctts_gpt_begin first)"); return 1; }
    if (!h->text_mode && !h->text_rows_on) { ctts_set_error("set_text_guide: a guide is for text rows: the call must be an infer_text call, or ctts_gpt_enable_text_rows must come first (a guide on a code row)"); return 1; }
    if (h->io.noise != nullptr && !h->text_mode) { ctts_set_error("set_text_guide: guides in a code call need device noise (caller-supplied noise is laid out for one mode's rows)"); return 1; }
    const SamplerCfgDev& tsc = h->text_mode ? h->sc : h->sc_text;
    if (check_free_ids("set_text_guide", free_ids, n_free, max_run, tsc.eos, h->vocab_text_head)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (!h->guide_tab && dev_alloc(h, (void**)&h->guide_tab, sizeof(GuideTab))) return 1;
    if (!h->guide_pin) {
        CTTS_HIP_CHECK(hipHostMalloc((void**)&h->guide_pin, (size_t)4 * GUIDE_PIN_INTS * 4, hipHostMallocDefault));
        for (hipEvent_t& e : h->guide_ev) CTTS_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // every slot starts unguided (n = 0); then the header
    CTTS_HIP_CHECK(hipMemsetAsync(h->guide_tab, 0, sizeof(GuideTab), s));
    int hdr[4 + CTTS_GUIDE_MAX_FREE] = {n_free, max_run, 0, 0};
    for (int i = 0; i < n_free; ++i) hdr[4 + i] = free_ids[i];
    CTTS_HIP_CHECK(hipMemcpyAsync(h->guide_tab, hdr, sizeof(hdr), hipMemcpyHostToDevice, s));       // pageable source: staged before the call returns
    GuideTab* const p = h->guide_tab;
    CTTS_HIP_CHECK(hipMemcpyAsync((char*)(h->text_mode ? h->dyn : h->dyn_text) + offsetof(SamplerDyn, guide), &p, sizeof(p), hipMemcpyHostToDevice, s));
    h->guide_len.assign(CTTS_GUIDE_SLOTS, 0);
    h->guide_on = 1;
    return 0;
}

extern "C" int ctts_gpt_set_guides(ctts_gpt* h, int n, const int32_t* out_slots, const int32_t* src_concat, const int32_t* src_off, void* stream) {
    if (!h || h->B == 0) { ctts_set_error("set_guides: no generate state (call ctts_gpt_begin first)"); return 1; }
    if (!h->guide_on) { ctts_set_error("set_guides: guides without the per-call part: call ctts_gpt_set_text_guide first (after ctts_gpt_begin / ctts_gpt_enable_text_rows)"); return 1; }
    if (n < 0 || (n > 0 && (!out_slots || !src_off))) { ctts_set_error("set_guides: bad argument"); return 1; }
    const SamplerCfgDev& tsc = h->text_mode ? h->sc : h->sc_text;
    const bool seated = !h->sampled && !h->admitted;      // begin's rows are still what finend_host describes
    for (int i = 0; i < n; ++i) {
        const int slot = out_slots[i], len = src_off[i + 1] - src_off[i];
        if (slot < 0 || slot >= CTTS_GUIDE_SLOTS) { ctts_set_error("set_guides: entry %d: output slot %d outside 0..%d (the guide table's extent)", i, slot, CTTS_GUIDE_SLOTS - 1); return 1; }
        if (len < 0 || (len > 0 && !src_concat)) { ctts_set_error("set_guides: entry %d: bad source extent", i); return 1; }
        if (len == 0) continue;
        int limit = tsc.max_new;
        if (seated)
            for (int b = 0; b < h->B && b < (int)h->finend_host.size(); ++b) {
                const RowState& r = h->finend_host[b];
                if (r.out != slot) continue;
                if (!h->text_mode && r.mode == 0) { ctts_set_error("set_guides: entry %d: output slot %d is held by a code row (a guide on a code row)", i, slot); return 1; }
                limit = r.limit < limit ? r.limit : limit;
            }
        if (check_guide_src("set_guides", i, src_concat + src_off[i], len, limit, tsc.eos, h->vocab_text_head)) return 1;
    }
    hipStream_t s = (hipStream_t)stream;
    int slot = -1, used = 0;
    auto close_slot = [&]() -> int {
        if (slot >= 0 && used > 0) { CTTS_HIP_CHECK(hipEventRecord(h->guide_ev[slot], s)); h->guide_pin_used[slot] = true; }
        return 0;
    };
    for (int i = 0; i < n; ++i) {
        const int len = src_off[i + 1] - src_off[i], ints = 4 + len;
        if (slot < 0 || used + ints > GUIDE_PIN_INTS) {
            if (close_slot()) return 1;
            slot = (int)(h->guide_pin_next++ % 4); used = 0;
            if (h->guide_pin_used[slot]) CTTS_HIP_CHECK(hipEventSynchronize(h->guide_ev[slot]));
        }
        int* p = h->guide_pin + (size_t)slot * GUIDE_PIN_INTS + used;
        p[0] = len; p[1] = 0; p[2] = 0; p[3] = 0;                      // a fresh record: cur = run = 0
        for (int k = 0; k < len; ++k) p[4 + k] = src_concat[src_off[i] + k];
        CTTS_HIP_CHECK(hipMemcpyAsync(&h->guide_tab->rec[out_slots[i]], p, (size_t)ints * 4, hipMemcpyHostToDevice, s));
        used += ints;
        h->guide_len[out_slots[i]] = len;
    }
    return close_slot();
}

extern "C" int ctts_gpt_sample(ctts_gpt* h, void* stream) {
    if (!h || h->B == 0) { ctts_set_error("sample: call begin first"); return 1; }
    if (h->text_live > 0 && !h->text_rows_on) { ctts_set_error("sample: a row of the batch is a text row (ctts_gpt_set_row_modes) but ctts_gpt_enable_text_rows has not been called for this generate state"); return 1; }
    CTTS_RANGE("ctts_gpt_sample");
    h->sampled = true;
    if (h->batch_inv) {          // the last prompt token's layer pass first (see prefill_invariant): a decode step
        if (ensure_persist_images(h)) return 1;
        return run_decode_step(h, pick_decode_path(h, 0), (hipStream_t)stream);
    }
    return run_sample_phase(h, plain_form(h), (hipStream_t)stream);
}

extern "C" int ctts_gpt_restart(ctts_gpt* h, void* stream) {
    if (!h || h->B == 0) { ctts_set_error("restart: call begin first"); return 1; }
    if (h->B != h->B0) { ctts_set_error("restart: rows were compacted away (a regenerate restarts the whole batch at step 0, gpt.py:496-525)"); return 1; }
    if (h->admitted) { ctts_set_error("restart: rows of this batch were handed to other utterances (ctts_gpt_admit); re-admit the utterance with attempt + 1 instead"); return 1; }
    if (h->text_rows_on || h->text_live > 0) { ctts_set_error("restart: text rows are enabled (ctts_gpt_enable_text_rows): a regenerate restarts the whole batch in one mode; re-admit the utterance with attempt + 1 instead"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    CTTS_HIP_CHECK(hipMemcpyAsync(h->x_dec, h->x_last, (size_t)h->B * h->H * 4, hipMemcpyDeviceToDevice, s));
    if (h->batch_inv) CTTS_HIP_CHECK(hipMemcpyAsync(h->rope_dec, h->rope_dec0, (size_t)h->B * 64 * 4, hipMemcpyDeviceToDevice, s));      // the first layer pass again
    return reset_state(h, true, s);
}

// host mirror of the decode rows' context lengths (an upper bound: a row stops growing when it finishes, at the latest at prompt + limit):
// the longest one after `n_steps` more steps picks the attention's key-split count
static int advance_rows(ctts_gpt* h, int n_steps) {
    int longest = 1;
    for (HostRow& r : h->rows) {
        r.ctx = std::min(r.ctx + n_steps, r.cap);
        if (r.ctx > longest) longest = r.ctx;
    }
    return longest;
}

// The steps about to be launched run their layers as persistent launches: small fp32 batches without per-utterance adapters whose longest context stays
// within what one workgroup per (row, head) serves.
// Returns the key splits per (row, head) (0 = launch chain): as many shares as keep every share within what a workgroup prefetches, at most 64 / (12 B) and
// PL_SMAX; a context beyond twice that many prefetchable keys goes back to the launch chain (its attention spreads the keys over up to 96 workgroups).
// Asked once per step (plan_decode): L is that step's longest context, so a step's share count does not depend on how its decode call was chunked.
static inline int decode_persist(const ctts_gpt* h, int B, int L) {
    const int rows = tuning(h).persist_rows;               // (batch_invariant: 0 -- the launch chain at every row count)
    if (!(rows > 0 && h->pimg != nullptr && B <= rows && B <= PL_MAXR)) return 0;
    if (h->lora_rows && h->lora_mlp) return 0;             // ... on the MLP projections: the launch carries q/k/v/o terms only (ctts_hip.h "persistent_lora")
    if (h->lora_rows && !(h->persist_lora && h->persist_sched == 3 && h->lora_Af != nullptr && h->H == PL_H)) return 0;      // per-utterance adapters ride inside the launch (round 6, paced schedule)
    int cap = PL_ATT_BLOCKS / (PL_NH * B);
    cap = cap > PL_SMAX ? PL_SMAX : (cap < 1 ? 1 : cap);
    if (h->persist_splits > 0) cap = h->persist_splits < cap ? h->persist_splits : cap;
    // (until round 5 a context beyond 2 * 384 * cap + 256 keys went back to the launch chain: the share's tail streamed one 64-key step per round trip.  Four steps
    //  per round trip now; "persistent_max_keys" restores a limit for A/Bs)
    // Measured (tools/long_ctx_probe.py, ms/step launch chain / persistent): 3 rows 1200 keys 0.702 / 0.644, 1900 keys 0.733 / 0.808; 4 rows 1200 keys 0.717 / 0.708,
    // 1900 keys 0.748 / 0.877; 2 rows (2 shares) 1900 keys 0.568 / 0.535; 1 row 1900 keys 0.504 / 0.364: one workgroup streams a share at ~40 GB/s, so a share
    // beyond ~1400 keys loses to the chain's 144 attention blocks -> the limit is 1400 keys per share
    if (B > PL_MAXR_ONE) {
        // 6..8 rows: two (row, head) items per attention workgroup, no key splits: 192 keys per item are requested before the query exists, the rest streams behind it
        // 128 keys per round trip -- the chain's 72..96 attention blocks win beyond a few such trips ("persistent_max_keys")
        if (h->persist_sched != 3) return 0;
        return (L > (h->persist_max_keys > 0 ? h->persist_max_keys : h->persist_pair_keys - 128 * (B - PL_MAXR_ONE - 1))) ? 0 : 1;      // (704 / 576 / 448 keys at 6 / 7 / 8 rows)
    }
    if (L > (h->persist_max_keys > 0 ? h->persist_max_keys : 1400 * cap)) return 0;
    const int share = h->persist_share_keys > 0 ? h->persist_share_keys : PL_SHARE_KEYS;
    if (L <= share + 128) return 1;                         // (the 128 keys beyond the registers wait in LDS since round 6: cheaper than the extra hop)
    const int want = (L + share - 1) / share;
    return want > cap ? cap : want;
}

static inline DecodePath pick_decode_path(const ctts_gpt* h, int longest) { return {decode_splits(h, h->B, longest), decode_persist(h, h->B, longest)}; }

// Persistent launches of ONE process on one device take turns.  Each needs all 256 workgroups resident; two of them enqueued on different streams (two engines, two
// threads: a base engine and a LoRA-merged sibling, two pipelines) could each be given a share of the CUs and wait for the other's until both give up.  The
// per-device file lock keeps OTHER processes off the mode; this keeps the process's own streams apart: a decode call that launches persistent kernels first makes its
// stream wait for the previous such call's last launch (an event, no host wait), then records its own.  Calls on one stream are ordered anyway.
struct PersistTurn {
    std::mutex mu;
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool pending = false;
};
static PersistTurn* persist_turn() {
    static std::mutex mu;
    static std::map<int, PersistTurn*> turns;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    auto it = turns.find(dev);
    if (it != turns.end()) return it->second;
    PersistTurn* t = new PersistTurn();
    if (hipEventCreateWithFlags(&t->ev, hipEventDisableTiming) != hipSuccess) { delete t; return nullptr; }
    turns[dev] = t;
    return t;
}
struct PersistTurnGuard {
    PersistTurn* t = nullptr;
    hipStream_t s = nullptr;
    int rc = 0;
    PersistTurnGuard(bool persistent, hipStream_t stream) : s(stream) {
        if (!persistent) return;
        t = persist_turn();
        if (!t) return;
        t->mu.lock();
        if (t->pending && t->last != s && hipStreamWaitEvent(s, t->ev, 0) != hipSuccess) rc = 1;
    }
    ~PersistTurnGuard() {
        if (!t) return;
        if (hipEventRecord(t->ev, s) == hipSuccess) { t->last = s; t->pending = true; }
        t->mu.unlock();
    }
};

static int run_decode_step(ctts_gpt* h, DecodePath path, hipStream_t s) {
    StreamForm form = {};
    if (run_layers(h, h->x_dec, h->meta_dec, h->rope_dec, h->B, path, h->st, s, &form)) return 1;
    return run_sample_phase(h, form, s);            // the heads add dpart[0..3] / read the packed copy; the sampler then re-materialises x_dec
}

// steps per replay of a decode path, given `left` steps to launch: the long graph of the persistent paths while it fits, else the short one
static int graph_span(const ctts_gpt* h, DecodePath path, int left) {
    return (path.persist && h->graph_steps_persist > h->graph_steps && left >= h->graph_steps_persist) ? h->graph_steps_persist : h->graph_steps;
}

static int ensure_graph(ctts_gpt* h, DecodePath path, int n_steps) {
    char sig[160];
    snprintf(sig, sizeof(sig), "%d|%d|%p|%d|%d|%d|%d|%d", h->B, h->text_mode + 2 * (h->text_live > 0 ? 1 : 0) + 4 * h->guide_on, (void*)h->kv, path.splits, h->lora_rows + 2 * h->lora_mlp, h->opt_gen, path.persist, n_steps);      // (+ 2: a mixed step, two more launches)      // (diagnostic switches are fixed at create)
    std::string key(sig);
    if (h->lora_rows) { signed char slots[CTTS_MAX_B]; row_slot_bytes(h, slots, h->B); key.append((const char*)slots, (size_t)h->B); }      // the rows' adapter slots are kernel arguments of the folded launches (LoraFold)
    if (h->graph_gen != h->opt_gen || h->graphs.size() >= 96) {
        // graphs captured under other option / adapter settings are dead weight (loading one adapter bumps opt_gen ~80 times), and the cache is bounded: a serving
        // process cycles through few (batch, mode) shapes.  Replays of the dropped graphs may still be in flight (generate() keeps two chunks enqueued): drain first.
        if (!h->graphs.empty()) {
            CTTS_HIP_CHECK(hipDeviceSynchronize());
            for (auto& kv : h->graphs) { (void)hipGraphExecDestroy(kv.second.exec); (void)hipGraphDestroy(kv.second.graph); }
            h->graphs.clear(); h->gexec = nullptr;
        }
        h->graph_gen = h->opt_gen;
    }
    auto it = h->graphs.find(key);
    if (it != h->graphs.end()) { h->gexec = it->second.exec; return 0; }
    ctts_gpt::GraphEntry ge = {nullptr, nullptr};
    CTTS_HIP_CHECK(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
    int rc = 0;
    for (int i = 0; i < n_steps && !rc; ++i) rc = run_decode_step(h, path, h->cap_stream);
    hipError_t e = hipStreamEndCapture(h->cap_stream, &ge.graph);
    if (rc) { if (ge.graph) (void)hipGraphDestroy(ge.graph); return 1; }
    if (e != hipSuccess) { ctts_set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); return 1; }
    e = hipGraphInstantiate(&ge.exec, ge.graph, nullptr, nullptr, 0);
    if (e != hipSuccess) { (void)hipGraphDestroy(ge.graph); ctts_set_error("hipGraphInstantiate: %s", hipGetErrorString(e)); return 1; }
    h->graphs[key] = ge;
    h->gexec = ge.exec;
    return 0;
}

// The decode path of every coming step (key splits, persistent share count) from THAT step's context alone: step i of the next n_steps sees the longest
// row after i steps (what a call of i steps would pick).  A generation then runs the same kernels at every step however its caller chunks the calls (one
// 512-step call used to run all its steps with the share count of its LAST context).  Consecutive steps with equal paths form one segment.
static void plan_decode(ctts_gpt* h, int n_steps) {
    h->segs.clear();
    for (int i = 1; i <= n_steps; ++i) {
        int longest = 1;
        for (const HostRow& r : h->rows) longest = std::max(longest, std::min(r.ctx + i, r.cap));
        const DecodePath path = pick_decode_path(h, longest + 1);
        if (!h->segs.empty() && h->segs.back().path.splits == path.splits && h->segs.back().path.persist == path.persist) ++h->segs.back().n;
        else h->segs.push_back({1, path});
    }
}

// one segment's steps: whole graph spans as replays, the rest (at most graph_steps - 1 steps) eagerly; launch = false: only capture the graphs
static int run_segment(ctts_gpt* h, const ctts_gpt::DecodeSeg& sg, bool graphs, bool launch, hipStream_t s) {
    int left = sg.n;
    if (graphs) {
        while (left >= h->graph_steps) {
            const int span = graph_span(h, sg.path, left);
            if (ensure_graph(h, sg.path, span)) return 1;
            for (; left >= span; left -= span) if (launch) CTTS_HIP_CHECK(hipGraphLaunch(h->gexec, s));
        }
    }
    if (launch) for (; left > 0; --left) if (run_decode_step(h, sg.path, s)) return 1;
    return 0;
}

extern "C" int ctts_gpt_decode(ctts_gpt* h, int n_steps, int use_graph, void* stream) {
    if (!h || h->B == 0) { ctts_set_error("decode: call begin first"); return 1; }
    if (h->text_live > 0 && !h->text_rows_on) { ctts_set_error("decode: a row of the batch is a text row (ctts_gpt_set_row_modes) but ctts_gpt_enable_text_rows has not been called for this generate state"); return 1; }
    CTTS_RANGE("ctts_gpt_decode");              // reference: nvtx "forward" per decode step + "execute" (trt_models/predictor.py:164)
    hipStream_t s = (hipStream_t)stream;
    h->sampled = true;
    if (ensure_persist_images(h)) return 1;
    if (n_steps < 1) { h->launched += n_steps; (void)advance_rows(h, n_steps); return 0; }
    plan_decode(h, n_steps);
    (void)advance_rows(h, n_steps);
    h->launched += n_steps;
    bool persistent = false;
    for (const auto& sg : h->segs) persistent = persistent || sg.path.persist != 0;
    PersistTurnGuard turn(persistent, s);
    if (turn.rc) { ctts_set_error("decode: hipStreamWaitEvent failed"); return 1; }
    for (const auto& sg : h->segs) if (run_segment(h, sg, use_graph != 0, true, s)) return 1;
    return 0;
}

extern "C" int ctts_gpt_progress(ctts_gpt* h, int32_t* steps_done, int32_t* all_finished, void* stream) {
    if (!h) { ctts_set_error("null handle"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    CTTS_HIP_CHECK(hipMemcpyAsync(h->host_pin, h->st, 16, hipMemcpyDeviceToHost, s));
    h->host_pin[12] = 0;
    if (h->pl_error) CTTS_HIP_CHECK(hipMemcpyAsync(h->host_pin + 12, h->pl_error, 4, hipMemcpyDeviceToHost, s));
    CTTS_HIP_CHECK(hipStreamSynchronize(s));
    if (steps_done) *steps_done = h->host_pin[0];
    if (all_finished) *all_finished = h->host_pin[2];
    if (h->host_pin[12] == 7) {
        ctts_set_error("per-utterance LoRA: a projection tile gave up waiting for its low-rank term (lora_worker.h); use options={'lora_fold': 0}");
        return 1;
    }
    if (h->host_pin[12] != 0) {
        ctts_set_error("persistent decode layer: a workgroup gave up waiting on edge %d (2 = q|k|v -> attention, 3 = attention -> o_proj, 4 = o_proj -> gate|up, "
                       "5 = gate|up -> down); is the GPU shared with another process?  Use options={'persistent_rows': 0}", h->host_pin[12]);
        return 1;
    }
    return 0;
}

extern "C" int ctts_gpt_progress_enqueue(ctts_gpt* h, int32_t* host_pinned4, void* stream) {
    if (!h || !host_pinned4) { ctts_set_error("progress_enqueue: null argument"); return 1; }
    CTTS_HIP_CHECK(hipMemcpyAsync(host_pinned4, h->st, 16, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return 0;
}

extern "C" int ctts_gpt_saturations(ctts_gpt* h, int32_t* count, void* stream) {
    if (!h || !count || !h->sat) { ctts_set_error("saturations: bad argument"); return 1; }
    CTTS_HIP_CHECK(hipMemcpyAsync(h->host_pin + 8, h->sat, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    CTTS_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    *count = h->host_pin[8];
    return 0;
}

extern "C" int ctts_gpt_rows_enqueue(ctts_gpt* h, int32_t* host_pinned_2B, void* stream) {
    if (!h || !host_pinned_2B || h->B == 0) { ctts_set_error("rows_enqueue: call begin first"); return 1; }
    CTTS_HIP_CHECK(hipMemcpy2DAsync(host_pinned_2B, 8, h->finend, sizeof(RowState), 8, h->B, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return 0;
}

extern "C" int ctts_gpt_compact(ctts_gpt* h, const int32_t* keep_rows, int n_keep, void* stream) {
    if (!h || !keep_rows || h->B == 0) { ctts_set_error("compact: call begin first"); return 1; }
    if (n_keep < 1 || n_keep > h->B) { ctts_set_error("compact: n_keep=%d of %d rows", n_keep, h->B); return 1; }
    for (int i = 0; i < n_keep; ++i)
        if (keep_rows[i] < 0 || keep_rows[i] >= h->B || (i > 0 && keep_rows[i] <= keep_rows[i - 1])) { ctts_set_error("compact: keep_rows must be ascending row indices < %d", h->B); return 1; }
    if (n_keep == h->B) return 0;
    hipStream_t s = (hipStream_t)stream;
    h->keep_host.assign(keep_rows, keep_rows + n_keep);
    CTTS_HIP_CHECK(hipMemcpyAsync(h->keep_dev, h->keep_host.data(), (size_t)n_keep * 4, hipMemcpyHostToDevice, s));
    if (launch_compact_rows(h->keep_dev, n_keep, h->H, h->x_dec, h->rope_dec, h->meta_dec, h->hist_ring, h->finend, h->knobs, h->cx, h->crope, h->cmeta, h->cring, h->cfin,
                            h->cknobs, h->st, s)) return 1;
    for (int i = 0; i < n_keep; ++i) h->rows[i] = h->rows[keep_rows[i]];      // (ascending: keep_rows[i] >= i)
    h->rows.resize(n_keep); h->B = n_keep;
    // a batch that dropped its last text row is an ordinary code batch again; the LoRA launches stay only while a live row carries an adapter
    return refresh_rows(h);
}

// Adapter slots of the utterances the NEXT ctts_gpt_admit call seats in `rows` (-1 = none); rows not named keep theirs.  The slot follows the row's KV
// lane (the prompt pass of the admitted rows looks it up by sequence, lora.hip) and the row itself (the decode launches carry the rows' slots in their
// arguments, lora_worker.h).  When no live row has an adapter any more the engine drops back to the plain launches.
extern "C" int ctts_gpt_admit_adapters(ctts_gpt* h, int n, const int32_t* rows, const int32_t* slots, void* stream) {
    if (!h || h->B == 0 || !rows || !slots) { ctts_set_error("admit_adapters: call begin first / null argument"); return 1; }
    if (h->lora_slot_host.empty()) h->lora_slot_host.assign(CTTS_MAX_B, -1);      // (the rows' slots are -1 then)
    bool any = false;
    for (int i = 0; i < n; ++i) {       // (one message for a row or a slot out of range)
        if (slots[i] >= CTTS_MAX_ADAPTERS || check_rows(h, "admit_adapters", 1, rows + i, false)) { ctts_set_error("admit_adapters: row %d / slot %d out of range", rows[i], slots[i]); return 1; }
        any = any || slots[i] >= 0;
    }
    if (any && h->batch_inv) { ctts_set_error("admit_adapters: per-utterance adapters are outside the %s contract; set the option to 0 or merge the adapter", inv_name(h)); return 1; }
    if (any && lora_ensure_storage(h)) return 1;
    for (int i = 0; i < n; ++i) {
        const int sl = slots[i] < 0 ? -1 : slots[i];
        h->rows[rows[i]].slot = sl;
        h->lora_slot_host[h->rows[rows[i]].seq] = sl;
    }
    if (h->lora_slot_of_seq)        // (pageable source: staged before the call returns)
        CTTS_HIP_CHECK(hipMemcpyAsync(h->lora_slot_of_seq, h->lora_slot_host.data(), CTTS_MAX_B * 4, hipMemcpyHostToDevice, (hipStream_t)stream));
    return refresh_rows(h);
}

// Continuous batching (no counterpart in the reference, whose slices run to their slowest row, pipeline:391-397 / gpt.py:527-546): `n` new
// utterances take over decode rows whose utterance has finished.  Their prompts (all tokens but the last) go through an ordinary prompt pass
// into the rows' KV lanes, starting at slot 0 of the lane; the last prompt token becomes the row's next decode input, so the next decode
// step produces the utterance's first token together with everybody else's next one.  The row's step counter, noise stream (utterance id,
// attempt), token limit and output index are its own (RowState), so an utterance's tokens do not depend on when or where it was admitted.
extern "C" int ctts_gpt_admit(ctts_gpt* h, int n, const int32_t* rows, int T, const int32_t* mask, const float* emb, const uint64_t* utt_ids,
                              const int32_t* row_limits, const int32_t* out_index, const int32_t* attempts, void* stream) {
    if (!h || h->B == 0) { ctts_set_error("admit: call begin first"); return 1; }
    const NextCall req = take_next_call(h);      // for THIS admission only, whether it goes through or fails below
    const std::vector<int>& share = req.share; const int share_P = req.share_P;
    if (!share.empty() && (int)share.size() != n) { ctts_set_error("admit: ctts_gpt_share_prompts named the prompts of %d sequences, this call seats n=%d", (int)share.size(), n); return 1; }
    if (!share.empty() && h->text_mode) { ctts_set_error("admit: shared prompt passes (ctts_gpt_share_prompts) are code mode only"); return 1; }
    const int P = share.empty() ? n : share_P;   // prompts: mask [P][T], emb [P][T][H]
    if (!rows || !mask || !emb || !utt_ids || !out_index) { ctts_set_error("admit: null argument"); return 1; }
    if (h->io.noise != nullptr) { ctts_set_error("admit: device noise only (caller-supplied noise is indexed by the batch's draw counter)"); return 1; }
    if (h->batch_inv && h->lora_rows) { ctts_set_error("admit: per-utterance adapters are outside the %s contract; set the option to 0 or merge the adapter", inv_name(h)); return 1; }
    if (n < 1 || n > h->B || T < 1 || T + h->sc.max_new > h->cfg.max_seq || (long long)P * (T - 1) > h->pass_rows) {
        ctts_set_error("admit: n=%d of %d rows on %d prompts, T=%d (max_seq %d; %d x %d prompt rows for %d per pass)", n, h->B, P, T, h->cfg.max_seq, P, T - 1, h->pass_rows);
        return 1;
    }
    CTTS_RANGE("ctts_gpt_admit");
    hipStream_t s = (hipStream_t)stream;
    h->keep_host.assign(rows, rows + n);
    std::vector<int>& seqs = h->seq_host;
    seqs.assign(n, 0);
    h->fresh_host.assign(n, RowState{});
    if (check_rows(h, "admit", n, rows, true, [&](int i) {
        seqs[i] = h->rows[rows[i]].seq;
        RowState& r = h->fresh_host[i];
        int lim = row_limits ? row_limits[i] : h->sc.max_new;
        r.limit = lim < 1 ? 1 : (lim > h->sc.max_new ? h->sc.max_new : lim);
        r.uid_lo = (unsigned)utt_ids[i]; r.uid_hi = (unsigned)(utt_ids[i] >> 32);
        r.attempt = attempts ? attempts[i] : 0;
        r.out = out_index[i];
        if (r.out < 0) { ctts_set_error("admit: negative output index"); return 1; }
        for (const auto& e : req.modes) if (e.first == rows[i]) r.mode = e.second;
        if (r.mode == 1) {
            if (!h->text_rows_on) { ctts_set_error("admit: row %d is to hold a text utterance (ctts_gpt_admit_modes) but ctts_gpt_enable_text_rows has not been called for this generate state", rows[i]); return 1; }
            if (!share.empty()) { ctts_set_error("admit: shared prompt passes (ctts_gpt_share_prompts) are for code rows; row %d is to hold a text utterance (ctts_gpt_admit_modes)", rows[i]); return 1; }
            for (const auto& e : req.knobs) if (e.first == rows[i]) {
                ctts_set_error("admit: row %d is to hold a text utterance (ctts_gpt_admit_modes) and carries per-row sampling knobs (ctts_gpt_admit_sampling); text rows keep the values of ctts_gpt_enable_text_rows", rows[i]);
                return 1;
            }
            if (r.limit > h->sc_text.max_new) r.limit = h->sc_text.max_new;      // the text ids array is [n_out][max_new_text][4]
        }
        // the guide ctts_gpt_set_guides named for the row's output slot: text rows only, and the source and its EOS fit the row's limit
        if (h->guide_on && r.out < CTTS_GUIDE_SLOTS && h->guide_len[r.out] > 0) {
            if (!h->text_mode && r.mode == 0) { ctts_set_error("admit: row %d is to hold a code utterance at output slot %d, which carries a guide (a guide on a code row)", rows[i], r.out); return 1; }
            if (h->guide_len[r.out] + 1 > r.limit) {
                ctts_set_error("admit: row %d: the guide at output slot %d has a source of %d ids and needs %d tokens (the source and EOS), the row's limit is %d", rows[i], r.out, h->guide_len[r.out], h->guide_len[r.out] + 1, r.limit);
                return 1;
            }
        }
        return 0;
    })) return 1;
    // the new rows' sampling knobs: what ctts_gpt_admit_sampling named for the row, else the call's values (never the finished utterance's)
    h->knobs_host.assign(n, knobs_of_cfg(h->sc));
    for (int i = 0; i < n; ++i)
        for (const auto& e : req.knobs) if (e.first == rows[i]) h->knobs_host[i] = e.second;
    if (!share.empty() && share_plan(h, share, P, seqs.data(), "admit", s)) return 1;
    int* rows_dev = h->keep_dev;
    int* seqs_dev = h->cring;                    // (compaction scratch: consumed in stream order)
    RowState* fresh_dev = h->cfin;
    CTTS_HIP_CHECK(hipMemcpyAsync(rows_dev, h->keep_host.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    CTTS_HIP_CHECK(hipMemcpyAsync(seqs_dev, seqs.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    CTTS_HIP_CHECK(hipMemcpyAsync(fresh_dev, h->fresh_host.data(), (size_t)n * sizeof(RowState), hipMemcpyHostToDevice, s));
    CTTS_HIP_CHECK(hipMemcpyAsync(h->cknobs, h->knobs_host.data(), (size_t)n * sizeof(RowSampling), hipMemcpyHostToDevice, s));
    AdmitArgs a = {};
    a.mask = mask; a.emb = emb; a.rows = rows_dev; a.seqs = seqs_dev; a.fresh = fresh_dev; a.n = n; a.T = T; a.H = h->H;
    a.fresh_knobs = h->cknobs; a.knobs = h->knobs;
    a.pm = h->meta_pre; a.rope_pre = h->rope_pre; a.dm = h->meta_dec; a.rope_dec = h->rope_dec; a.x_dec = h->x_dec; a.ring = h->hist_ring; a.finend = h->finend;
    a.rope = h->rope; a.st = h->st; a.finish = h->io.finish; a.end_idx = h->io.end_idx; a.share = share.empty() ? nullptr : h->share_dev;
    if (launch_admit_rows(a, s)) return 1;
    const long R = (long)P * (T - 1);
    if (R > 0) {
        // prompt rows [P][T-1] <- emb[i][0 .. T-2]: one pass (R <= pass_rows was checked above), which leaves the "prompt_plan" of the last prefill as it is
        if (prompt_passes(h, R, T - 1, s, [&](long r0, int m) { return stage_rows_but_last(h, emb, T, r0, m, s); }, no_after)) return 1;
        if (!share.empty() && share_kv(h, T - 1, s)) return 1;      // the followers' lanes <- the leaders' span [0, T - 1)
    }
    // the rows' records: the lane and the adapter slot (ctts_gpt_admit_adapters) stay, the rest is the new utterance's (a row handed to a code utterance stops counting as a text row here)
    for (int i = 0; i < n; ++i) { HostRow& r = h->rows[rows[i]]; r.ctx = T; r.cap = T + h->fresh_host[i].limit; r.mode = h->fresh_host[i].mode; }
    h->admitted = true;
    return refresh_rows(h);
}

// Elastic batch (no counterpart in the reference): n dead rows behind the decode batch, for the ctts_gpt_admit that follows.  A dead row runs through the layers
// and appends K / V at slot 0 of its lane, so it gets a lane no row of the batch holds: the lowest free ones (after a compaction those are not B ..).  h->B changes
// exactly as in ctts_gpt_compact: the next ctts_gpt_decode plans, picks its graphs and its persistent launches by the new row count.
extern "C" int ctts_gpt_grow(ctts_gpt* h, int n, void* stream) {
    if (!h || h->B == 0) { ctts_set_error("grow: no generate state (call ctts_gpt_begin first)"); return 1; }
    if (h->io.noise != nullptr) { ctts_set_error("grow: device noise only (caller-supplied noise is indexed by the batch's draw counter and sized for the rows of begin)"); return 1; }
    if (n < 1) { ctts_set_error("grow: n=%d (at least one row)", n); return 1; }
    if (h->B + n > h->cfg.max_batch) { ctts_set_error("grow: %d + %d rows exceed max_batch=%d", h->B, n, h->cfg.max_batch); return 1; }
    CTTS_RANGE("ctts_gpt_grow");
    hipStream_t s = (hipStream_t)stream;
    const int B = h->B;
    bool used[CTTS_MAX_B] = {};
    for (const HostRow& r : h->rows) used[r.seq] = true;
    h->seq_host.assign(n, 0);
    for (int i = 0, lane = 0; i < n; ++i, ++lane) {
        while (used[lane]) ++lane;               // (B + n <= max_batch and the rows' lanes are distinct: n free lanes exist below max_batch)
        h->seq_host[i] = lane;
        if (!h->lora_slot_host.empty()) h->lora_slot_host[lane] = -1;
    }
    if (!h->lora_slot_host.empty() && h->lora_slot_of_seq)
        CTTS_HIP_CHECK(hipMemcpyAsync(h->lora_slot_of_seq, h->lora_slot_host.data(), CTTS_MAX_B * 4, hipMemcpyHostToDevice, s));
    h->knobs_host.assign(1, knobs_of_cfg(h->sc));
    CTTS_HIP_CHECK(hipMemcpyAsync(h->keep_dev, h->seq_host.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));      // (compaction scratch: consumed in stream order)
    CTTS_HIP_CHECK(hipMemcpyAsync(h->cknobs, h->knobs_host.data(), sizeof(RowSampling), hipMemcpyHostToDevice, s));
    GrowArgs a = {};
    a.B0 = B; a.n = n; a.H = h->H; a.seqs = h->keep_dev;
    a.dm = h->meta_dec; a.rope_dec = h->rope_dec; a.x_dec = h->x_dec; a.ring = h->hist_ring; a.finend = h->finend;
    a.knobs = h->knobs; a.call_knobs = h->cknobs; a.rope = h->rope; a.st = h->st;
    if (launch_grow_rows(a, s)) return 1;
    for (int i = 0; i < n; ++i) h->rows.push_back(HostRow{h->seq_host[i], 1, 1, 0, -1});      // parked on slot 0 of its lane; a dead row is a code row without an adapter
    h->B = B + n;
    h->admitted = true;                          // x_last / meta_dec0 no longer describe the rows: no ctts_gpt_restart
    return refresh_rows(h);
}

// Ends the utterances in `rows` where they stand (a client went away): the rows become ordinary finished rows -- they write nothing more, rows_enqueue reports
// them, admit may take them, compact may drop them.  The row count does not change, so the other rows' launches are those of the same schedule without the call.
extern "C" int ctts_gpt_cancel(ctts_gpt* h, int n, const int32_t* rows, void* stream) {
    if (!h || h->B == 0) { ctts_set_error("cancel: no generate state (call ctts_gpt_begin first)"); return 1; }
    if (n < 1 || !rows) { ctts_set_error("cancel: n=%d rows / null argument", n); return 1; }
    if (check_rows(h, "cancel", n, rows, true)) return 1;
    CTTS_RANGE("ctts_gpt_cancel");
    hipStream_t s = (hipStream_t)stream;
    h->keep_host.assign(rows, rows + n);
    CTTS_HIP_CHECK(hipMemcpyAsync(h->keep_dev, h->keep_host.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    return launch_cancel_rows(h->keep_dev, n, h->finend, h->st, s);
}

// Diagnostics: copies a named internal buffer to HOST memory (tools/persist_probe.py compares the persistent layer's intermediates with the
// launch path's).  Synchronises the stream.  Returns the number of bytes copied through *bytes.
// GEMM kinds of debug_read "prompt_plan": launch_gemm with the norm in the block / on the packed operand, prefill_gemm.hip shape 0 / 1 / 2, prefill_split.hip SP_SHAPE_*
enum { PP_TILE_NORM = 0, PP_TILE_PACKED = 1, PP_PFG_0 = 2, PP_SPLIT_64 = 5 };
extern "C" int ctts_gpt_debug_read(ctts_gpt* h, const char* name, void* out, size_t max_bytes, size_t* bytes, void* stream) {
    if (!h || !name || !out) { ctts_set_error("debug_read: null argument"); return 1; }
    const std::string n(name);
    const void* src = nullptr; size_t nb = 0;
    if (n == "x_dec") { src = h->x_dec; nb = (size_t)CTTS_MAX_B * h->H * 4; }
    else if (n == "q_buf") { src = h->q_buf; nb = (size_t)32 * h->H * 4; }
    else if (n == "meta_dec") { src = h->meta_dec; nb = (size_t)CTTS_MAX_B * sizeof(RowMeta); }      // {KV lane, pos, slot, kv_start} per decode row
    else if (n == "logits") { src = h->logits; nb = (size_t)CTTS_MAX_B * h->NVQ * h->V * 4; }
    else if (n == "pl_g" && h->pl_g) { src = h->pl_g; nb = (size_t)PL_G_TOTAL * 8; }
    else if (n == "pl_ts" && h->pl_ts) { src = h->pl_ts; nb = (size_t)PL_BLOCKS * 10 * 8; }
    else if (n == "xh") { src = h->xh; nb = (size_t)2 * 48 * 1024; }
    else if (n == "ssq") { src = h->ssq; nb = (size_t)32 * 48 * 4; }
    else if (n == "guide_tab" && h->guide_tab) { src = h->guide_tab; nb = sizeof(GuideTab); }        // header, free ids, one 4 KB record {n, -, cur, run, src...} per output slot
    else if (n == "pl_state" && h->pl_epoch) {
        unsigned* o = (unsigned*)out;
        if (max_bytes < 8) { ctts_set_error("debug_read: buffer too small"); return 1; }
        CTTS_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
        CTTS_HIP_CHECK(hipMemcpy(o, h->pl_epoch, 4, hipMemcpyDeviceToHost));
        CTTS_HIP_CHECK(hipMemcpy(o + 1, h->pl_error, 4, hipMemcpyDeviceToHost));
        if (bytes) *bytes = 8;
        return 0;
    }
    else if (n == "decode_plan") {
        // host only: what plan_layers decides for the current batch on the path of the last planned decode step (no device work, nothing synchronised)
        if (h->B == 0 || h->segs.empty()) { ctts_set_error("debug_read: decode_plan: no decode call has been planned for this batch"); return 1; }
        const DecodePath path = h->segs.back().path;
        const LayerPlan p = plan_layers(h, h->B, true, path);
        const int32_t v[] = {h->B, path.splits, path.persist, p.S, p.nbg, p.chunks, p.dts, p.pf_kb, p.valu, p.wide_blocks, p.splitd, p.prepack, p.xhm, p.spd, p.down_sk,
                             p.fuse_heads, p.lora, p.form.parts, p.form.xh, p.form.logits, p.form.split, p.form.nbg, p.form.valu};
        if (max_bytes < sizeof(v)) { ctts_set_error("debug_read: buffer too small"); return 1; }
        memcpy(out, v, sizeof(v));
        if (bytes) *bytes = sizeof(v);
        return 0;
    }
    else if (n == "prompt_plan" || n == "meta_pre" || n == "x_pre") {
        // the passes of the last ctts_gpt_prefill / ctts_gpt_score call: full passes of pass_rows rows, then the rest
        if (h->pp_rows <= 0) { ctts_set_error("debug_read: %s: no prompt pass has run since begin", name); return 1; }
        const int passes = (int)((h->pp_rows + h->pass_rows - 1) / h->pass_rows), n_last = (int)(h->pp_rows - (long)(passes - 1) * h->pass_rows);
        if (n == "meta_pre") { src = h->meta_pre; nb = (size_t)h->pp_rows * sizeof(RowMeta); }      // {KV lane, pos, slot, kv_start} of every prompt row of the call
        else if (n == "x_pre") { src = h->x_pre; nb = (size_t)n_last * h->H * 4; }                  // the fp32 residual rows the last pass left
        else {
            // host only: what plan_layers and the launchers' own choice functions (kernels.h) decide at the two pass heights (no device work, nothing synchronised)
            const int n_full = passes > 1 ? h->pass_rows : n_last;
            int32_t v[4 + 2 * 15], k = 0;
            v[k++] = passes; v[k++] = n_full; v[k++] = n_last; v[k++] = h->pp_T;
            for (const int R : {n_full, n_last}) {
                const LayerPlan p = plan_layers(h, R, false, DecodePath{1, 0});
                const SplitGemmPolicy pol = {h->prefill_pp_blocks, p.prefill_sk_rows, h->sk_scratch, h->sk_cap_floats, h->prefill_small_blocks, h->prefill_ring4_blocks};
                const int32_t head[] = {p.nbg, p.prepack, p.pfg, p.pfs, p.anchor, p.lora, prompt_attention_kind(h->cfg.dtype, R, h->pp_T, p.anchor, p.pfs && p.S == 1)};
                for (const int32_t x : head) v[k++] = x;
                // the four projections as run_layers launches them: {epilogue, n tiles, k tiles, low-rank term present, reads the normalised residual rows}
                const struct { int epi, nt, kt; bool lora, norm; } proj[4] = {{EPI_QKV, 3 * h->H / 16, h->H / 32, p.lora, true}, {EPI_RESID, h->H / 16, h->H / 32, p.lora, false},
                                                                              {EPI_SWIGLU, 2 * h->I / 16, h->H / 32, p.lmlp, true}, {EPI_RESID, h->H / 16, h->I / 32, p.lmlp, false}};
                for (const auto& j : proj) {
                    int kind = (j.norm && !p.prepack) ? PP_TILE_NORM : PP_TILE_PACKED, sliced = 0;
                    if (p.pfs) { const SplitGemmShape c = split_gemm_shape(j.epi, R, j.nt, j.kt, j.lora, pol); kind = PP_SPLIT_64 + c.shape; sliced = c.sliced; }
                    else if (p.pfg) kind = PP_PFG_0 + prefill_gemm_shape(j.epi, R, p.pfg_shape);
                    v[k++] = kind; v[k++] = sliced;
                }
            }
            if (max_bytes < sizeof(v)) { ctts_set_error("debug_read: buffer too small"); return 1; }
            memcpy(out, v, sizeof(v));
            if (bytes) *bytes = sizeof(v);
            return 0;
        }
    }
    if (!src) { ctts_set_error("debug_read: unknown or unallocated buffer '%s'", name); return 1; }
    if (nb > max_bytes) nb = max_bytes;
    CTTS_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    CTTS_HIP_CHECK(hipMemcpy(out, src, nb, hipMemcpyDeviceToHost));
    if (bytes) *bytes = nb;
    return 0;
}

extern "C" int ctts_gpt_logits(ctts_gpt* h, float* out, void* stream) {
    if (!h || !out || h->B == 0) { ctts_set_error("logits: call begin first"); return 1; }
    CTTS_HIP_CHECK(hipMemcpyAsync(out, h->logits, (size_t)h->B * (h->text_mode ? h->vocab_text_head : h->NVQ * h->V) * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int ctts_gpt_force_ids(ctts_gpt* h, const int32_t* ids, void* stream) {
    if (!h || !ids || h->B == 0) { ctts_set_error("force_ids: call begin first"); return 1; }
    return launch_embed_ids(ids, h->emb_code, h->x_dec, h->B, h->V, h->H, (hipStream_t)stream);
}

// Stand-alone sampler (ctts_sampler_run / ctts_sampler_run_rows): the kernels read their configuration -- and the per-sequence knobs -- from device
// memory, a small ring of slots, one per call in flight.  per_seq == nullptr: every row uses the knobs of `sc`.
static int sampler_run_standalone(const ctts_sampler_cfg* sc, const ctts_row_sampling* per_seq, const float* logits, const int32_t* history, int hist_len,
                                  const float* q, int rows, int vocab, int step, int32_t* idx, float* lp_raw, float* lp_sampled, void* stream, const char* who) {
    if (!sc || !logits || !q || !idx || (hist_len > 0 && !history)) { ctts_set_error("%s: null argument", who); return 1; }
    const int nseq = (rows + CTTS_NUM_VQ - 1) / CTTS_NUM_VQ;
    if (per_seq) {
        if (rows < 1 || nseq > CTTS_MAX_B) { ctts_set_error("%s: rows=%d (at most %d sequences of 4 rows)", who, rows, CTTS_MAX_B); return 1; }
        for (int i = 0; i < nseq; ++i) if (check_knobs(per_seq[i], sc->max_new_token, who, i)) return 1;
    }
    static std::mutex mu;
    static SamplerDyn* ring = nullptr;
    static RowSampling* kring = nullptr;
    static unsigned next = 0;
    const unsigned NSLOT = 64;
    unsigned k;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!ring) CTTS_HIP_CHECK(hipMalloc((void**)&ring, NSLOT * sizeof(SamplerDyn)));
        if (per_seq && !kring) CTTS_HIP_CHECK(hipMalloc((void**)&kring, (size_t)NSLOT * CTTS_MAX_B * sizeof(RowSampling)));
        k = next++ % NSLOT;
    }
    SamplerDyn d = {};
    d.cfg = cfg_of_abi(*sc);
    d.noise = q;
    CTTS_HIP_CHECK(hipMemcpyAsync(ring + k, &d, sizeof(d), hipMemcpyHostToDevice, (hipStream_t)stream));       // pageable sources: staged before the call returns
    SamplerArgs sa = {};
    sa.dyn = ring + k;
    sa.logits = logits; sa.V = vocab; sa.B = rows; sa.st = nullptr; sa.history = history; sa.hist_len = hist_len;
    sa.step_override = step; sa.idx_out = idx; sa.lp_raw_out = lp_raw; sa.lp_sampled_out = lp_sampled;
    if (per_seq) {
        std::vector<RowSampling> tab(nseq);
        for (int i = 0; i < nseq; ++i) tab[i] = knobs_of_abi(per_seq[i]);
        sa.seq_knobs = kring + (size_t)k * CTTS_MAX_B;
        CTTS_HIP_CHECK(hipMemcpyAsync(kring + (size_t)k * CTTS_MAX_B, tab.data(), (size_t)nseq * sizeof(RowSampling), hipMemcpyHostToDevice, (hipStream_t)stream));
    }
    return launch_sampler(sa, nseq, (hipStream_t)stream);
}

extern "C" int ctts_sampler_run(const ctts_sampler_cfg* sc, const float* logits, const int32_t* history, int hist_len, const float* q,
                                int rows, int vocab, int step, int32_t* idx, void* stream) {
    return sampler_run_standalone(sc, nullptr, logits, history, hist_len, q, rows, vocab, step, idx, nullptr, nullptr, stream, "sampler_run");
}

extern "C" int ctts_sampler_run_rows(const ctts_sampler_cfg* sc, const ctts_row_sampling* per_seq, const float* logits, const int32_t* history, int hist_len,
                                     const float* q, int rows, int vocab, int step, int32_t* idx, void* stream) {
    if (!per_seq) { ctts_set_error("sampler_run_rows: null argument"); return 1; }
    return sampler_run_standalone(sc, per_seq, logits, history, hist_len, q, rows, vocab, step, idx, nullptr, nullptr, stream, "sampler_run_rows");
}

extern "C" int ctts_sampler_run_rows_lp(const ctts_sampler_cfg* sc, const ctts_row_sampling* per_seq, const float* logits, const int32_t* history, int hist_len,
                                        const float* q, int rows, int vocab, int step, int32_t* idx, float* lp_raw, float* lp_sampled, void* stream) {
    if (!per_seq) { ctts_set_error("sampler_run_rows_lp: null argument"); return 1; }
    return sampler_run_standalone(sc, per_seq, logits, history, hist_len, q, rows, vocab, step, idx, lp_raw, lp_sampled, stream, "sampler_run_rows_lp");
}

// Stand-alone guided text sampler (a test hook, synchronous): one step of sampler_text_kernel<true> -- the generate kernel itself, not a copy of its arithmetic -- on
// a one-step state built here: row r is a live text row at output slot r, at its own step, with its guide record at the given cursor.  Host arrays in, host arrays out.
// `guided` = false (ctts_sampler_run_text_lp without a source): sampler_text_kernel<false> on rows without records.  lp_raw_out / lp_sampled_out (host, [rows], either
// may be null): the log-probs the step wrote next to the id (ctts_gpt_set_text_logprob_out); both null = the launch of a call without the feature.
static int run_text_step(const char* who, bool guided, const ctts_sampler_cfg* sc, const float* logits, const float* q, int rows, int vocab, const int32_t* free_ids, int n_free,
                         int max_run, const int32_t* src_concat, const int32_t* src_off, const int32_t* cur, const int32_t* run, const int32_t* step,
                         const int32_t* limit, int32_t* idx_out, int32_t* cur_out, int32_t* run_out, float* lp_raw_out, float* lp_sampled_out, void* stream) {
    if (!sc || !logits || !q || !step || !limit || !idx_out) { ctts_set_error("%s: null argument", who); return 1; }
    if (guided && (!src_concat || !src_off || !cur || !run || !cur_out || !run_out)) { ctts_set_error("%s: null argument", who); return 1; }
    if (rows < 1 || rows > CTTS_GUIDE_SLOTS) { ctts_set_error("%s: rows=%d outside 1..%d", who, rows, CTTS_GUIDE_SLOTS); return 1; }
    if (!sc->infer_text || sc->use_penalty) { ctts_set_error("%s: sc must be the refine-text pass's parameters (infer_text = 1, no repetition penalty)", who); return 1; }
    if (vocab < 1 || sc->eos_token < 0 || sc->eos_token >= vocab) { ctts_set_error("%s: eos out of range", who); return 1; }
    if (vocab > 1024 * 21) { ctts_set_error("%s: vocab %d > %d", who, vocab, 1024 * 21); return 1; }
    if (guided && check_free_ids(who, free_ids, n_free, max_run, sc->eos_token, vocab)) return 1;
    int max_new = 1;
    for (int r = 0; r < rows; ++r) {
        if (limit[r] < 1 || limit[r] > 4096) { ctts_set_error("%s: row %d: limit %d outside 1..4096", who, r, limit[r]); return 1; }
        if (step[r] < 0 || step[r] >= limit[r]) { ctts_set_error("%s: row %d: step=%d outside 0..limit-1 (limit=%d)", who, r, step[r], limit[r]); return 1; }
        max_new = limit[r] > max_new ? limit[r] : max_new;
        if (!guided) continue;
        const int n = src_off[r + 1] - src_off[r];
        if (n < 1) { ctts_set_error("%s: row %d: a source of %d ids (n == 0 is an unguided row: not served by this hook)", who, r, n); return 1; }
        if (check_guide_src(who, r, src_concat + src_off[r], n, limit[r], sc->eos_token, vocab)) return 1;
        if (cur[r] < 0 || cur[r] > n || run[r] < 0) { ctts_set_error("%s: row %d: cur=%d run=%d step=%d outside the guide (n=%d, limit=%d)", who, r, cur[r], run[r], step[r], n, limit[r]); return 1; }
    }
    hipStream_t s = (hipStream_t)stream;
    // one scratch block: [guide header + rows records][SamplerDyn][DevState][RowState x rows][RowMeta x rows][rope 2 x 64][rope rows][ids][finish][end_idx][x_next][lp_raw][lp_sampled]
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t o_tab = 0, o_dyn = up(offsetof(GuideTab, rec) + (size_t)rows * sizeof(GuideRec)), o_st = o_dyn + up(sizeof(SamplerDyn)), o_rs = o_st + up(sizeof(DevState)),
                 o_meta = o_rs + up((size_t)rows * sizeof(RowState)), o_rope = o_meta + up((size_t)rows * sizeof(RowMeta)), o_rr = o_rope + up(128 * 4),
                 o_ids = o_rr + up((size_t)rows * 64 * 4), o_fin = o_ids + up((size_t)rows * max_new * CTTS_NUM_VQ * 4), o_end = o_fin + up((size_t)rows * 4),
                 o_x = o_end + up((size_t)rows * 4), o_lp = o_x + 256, lp_bytes = up((size_t)rows * max_new * 4), total = o_lp + 2 * lp_bytes;
    std::vector<char> img(o_rope, 0);                       // host image of everything up to the RoPE table; the rest is zero-filled on the device
    GuideTab* ht = (GuideTab*)(img.data() + o_tab);
    if (guided) {
        ht->n_free = n_free; ht->max_run = max_run;
        for (int i = 0; i < n_free; ++i) ht->free_ids[i] = free_ids[i];
    }
    RowState* hr = (RowState*)(img.data() + o_rs);
    for (int r = 0; r < rows; ++r) {
        if (guided) {
            GuideRec& g = ht->rec[r];
            g.n = src_off[r + 1] - src_off[r]; g.cur = cur[r]; g.run = run[r];
            for (int k = 0; k < g.n; ++k) g.src[k] = src_concat[src_off[r] + k];
        }
        hr[r].end = step[r]; hr[r].limit = limit[r]; hr[r].out = r; hr[r].uid_lo = (unsigned)r;
    }
    char* dev = nullptr;
    CTTS_HIP_CHECK(hipMalloc((void**)&dev, total));
    int rc = 1;
    do {
        SamplerDyn d = {};
        d.cfg = cfg_of_abi(*sc); d.cfg.max_new = max_new; d.n_draws = 1; d.ids = (int*)(dev + o_ids); d.finish = (int*)(dev + o_fin); d.end_idx = (int*)(dev + o_end);
        d.noise = q; d.rows0 = rows; d.guide = guided ? (GuideTab*)(dev + o_tab) : nullptr;
        d.lp_raw = lp_raw_out ? (float*)(dev + o_lp) : nullptr; d.lp_sampled = lp_sampled_out ? (float*)(dev + o_lp + lp_bytes) : nullptr;
        memcpy(img.data() + o_dyn, &d, sizeof(d));
        DevState* hs = (DevState*)(img.data() + o_st);
        hs->B = rows;
        if (hipMemsetAsync(dev + o_rope, 0, total - o_rope, s) != hipSuccess || hipMemcpyAsync(dev, img.data(), o_rope, hipMemcpyHostToDevice, s) != hipSuccess) { ctts_set_error("%s: upload failed", who); break; }
        SamplerArgs sa = {};
        sa.dyn = (const SamplerDyn*)(dev + o_dyn); sa.logits = logits; sa.V = vocab; sa.B = rows; sa.st = (DevState*)(dev + o_st);
        sa.text_mode = 1; sa.mixed = 0; sa.guided = guided ? 1 : 0;
        sa.emb_code = logits; sa.H = 0; sa.x_next = (float*)(dev + o_x);            // H = 0: no next-input row is written
        sa.meta = (RowMeta*)(dev + o_meta); sa.rope = (const float*)(dev + o_rope); sa.rope_rows = (float*)(dev + o_rr); sa.finend = (RowState*)(dev + o_rs);
        if (launch_sampler(sa, rows, s)) break;
        std::vector<int> ids((size_t)rows * max_new * CTTS_NUM_VQ);
        std::vector<float> lps(2 * lp_bytes / 4);
        if (hipMemcpyAsync(ids.data(), dev + o_ids, ids.size() * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(lps.data(), dev + o_lp, 2 * lp_bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(img.data(), dev + o_tab, o_dyn, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
            ctts_set_error("%s: %s", who, hipGetErrorString(hipGetLastError()));
            break;
        }
        for (int r = 0; r < rows; ++r) {
            idx_out[r] = ids[((size_t)r * max_new + step[r]) * CTTS_NUM_VQ];
            if (guided) { cur_out[r] = ht->rec[r].cur; run_out[r] = ht->rec[r].run; }
            if (lp_raw_out) lp_raw_out[r] = lps[(size_t)r * max_new + step[r]];
            if (lp_sampled_out) lp_sampled_out[r] = lps[lp_bytes / 4 + (size_t)r * max_new + step[r]];
        }
        rc = 0;
    } while (false);
    (void)hipStreamSynchronize(s);
    (void)hipFree(dev);
    return rc;
}
extern "C" int ctts_sampler_run_text_guided(const ctts_sampler_cfg* sc, const float* logits, const float* q, int rows, int vocab, const int32_t* free_ids, int n_free,
                                            int max_run, const int32_t* src_concat, const int32_t* src_off, const int32_t* cur, const int32_t* run, const int32_t* step,
                                            const int32_t* limit, int32_t* idx_out, int32_t* cur_out, int32_t* run_out, void* stream) {
    if (!src_concat) { ctts_set_error("sampler_run_text_guided: null argument"); return 1; }
    return run_text_step("sampler_run_text_guided", true, sc, logits, q, rows, vocab, free_ids, n_free, max_run, src_concat, src_off, cur, run, step, limit, idx_out, cur_out,
                         run_out, nullptr, nullptr, stream);
}
// The same step with the log-probs of the returned id (a test hook, synchronous).  src_concat == NULL: unguided rows through sampler_text_kernel<false> (the guide
// arguments and cur_out / run_out are ignored); otherwise the guided instantiation as above.
extern "C" int ctts_sampler_run_text_lp(const ctts_sampler_cfg* sc, const float* logits, const float* q, int rows, int vocab, const int32_t* free_ids, int n_free,
                                        int max_run, const int32_t* src_concat, const int32_t* src_off, const int32_t* cur, const int32_t* run, const int32_t* step,
                                        const int32_t* limit, int32_t* idx_out, int32_t* cur_out, int32_t* run_out, float* lp_raw_out, float* lp_sampled_out, void* stream) {
    return run_text_step("sampler_run_text_lp", src_concat != nullptr, sc, logits, q, rows, vocab, free_ids, n_free, max_run, src_concat, src_off, cur, run, step, limit,
                         idx_out, cur_out, run_out, lp_raw_out, lp_sampled_out, stream);
}

extern "C" int ctts_gpt_time_decode(ctts_gpt* h, int n_steps, float* ms_per_step, void* stream) {
    if (!h || h->B == 0 || n_steps < 1 || !ms_per_step) { ctts_set_error("time_decode: bad argument"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    // the steps run as ctts_gpt_decode runs them (plan_decode: each step's path from its own context); the graphs of every segment are captured
    // before the clock starts
    n_steps = (n_steps + h->graph_steps - 1) / h->graph_steps * h->graph_steps;
    h->sampled = true;
    if (ensure_persist_images(h)) return 1;
    plan_decode(h, n_steps);
    for (const auto& sg : h->segs) if (run_segment(h, sg, true, false, s)) return 1;
    CTTS_HIP_CHECK(hipEventRecord(h->ev0, s));
    for (const auto& sg : h->segs) if (run_segment(h, sg, true, true, s)) return 1;
    (void)advance_rows(h, n_steps);
    h->launched += n_steps;
    CTTS_HIP_CHECK(hipEventRecord(h->ev1, s));
    CTTS_HIP_CHECK(hipEventSynchronize(h->ev1));
    float ms = 0.f;
    CTTS_HIP_CHECK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *ms_per_step = ms / n_steps;
    return 0;
}

extern "C" double ctts_gpt_step_bytes(const ctts_gpt* h, int B, double mean_ctx) {
    // s * [ W + B*(L+1)*KV_tok ],  W = layers*(4H^2 + 3HI) + 4*V*H + (2*layers+1)*H
    const double W = (double)h->L * (4.0 * h->H * h->H + 3.0 * h->H * h->I) + (double)h->NVQ * h->V * h->H + (2.0 * h->L + 1) * h->H;
    const double kv_tok = (double)h->L * 2 * h->H;
    return h->esz * (W + B * (mean_ctx + 1.0) * kv_tok);
}
