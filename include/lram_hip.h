/*
 * lram_hip.h -- C ABI of the MI355X-native recurrent action-inference engine.
 *
 * The reference (ml-jku/LRAM) has no C interface: its drop-in boundary for the rollout hot path is the
 * Python `self.encoder(inputs_embeds, past_key_values, use_cache)` operator of the policy
 * (src/algos/models/decision_xlstm.py:138-169, src/algos/models/decision_mamba.py:109-166) together
 * with the embed / head code around it (src/algos/models/online_decision_transformer_model.py:392-461).
 * Each entry point below names the reference interface it stands in for.  Host code (the lram_amd package)
 * binds this library with ctypes; INTEGRATION.md shows the stub a maintainer adds on the LRAM side.
 *
 * Conventions
 *   - plain C, no torch / C++ types; every pointer argument says host or device.
 *   - every function returns 0 on success, non-zero on error; lram_last_error() gives the text.
 *   - one engine = one GPU, one stream per call (caller passes a hipStream_t as void*, NULL = default
 *     stream); no internal threads; calls on one engine must be externally serialised.
 *   - all floating point data is fp32, row-major, contiguous unless a stride is given.
 */
#ifndef LRAM_HIP_H
#define LRAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRAM_ABI_VERSION 1

#define LRAM_BACKBONE_XLSTM 0
#define LRAM_BACKBONE_MAMBA 1

#define LRAM_MAX_BLOCKS 64

/* Mixed-domain batches (lram_set_slot_table below) */
#define LRAM_HEAD_PER_SLOT 2 /* value of `discrete`: take the head mode of each slot from the slot table */
#define LRAM_SLOT_DISCRETE 1 /* flags[b] bit 0: discrete head (first n_discrete logits of action dim 0, action = index) */
#define LRAM_SLOT_IMAGE    2 /* flags[b] bit 1: the slot's observation is a uint8 frame */

/* Model description.  Mirrors the fields the reference reads from `agent_params.huggingface`
 * (configs/agent_params/huggingface/xlstm_*.yaml, mamba_*.yaml -> xLSTMConfig / MambaConfig,
 * src/algos/models/decision_xlstm.py:104-116, src/algos/models/decision_mamba.py:15-49) and from
 * `agent_params.model_kwargs` (configs/agent_params/model_kwargs/multi_domain.yaml). */
typedef struct lram_config {
  int32_t abi_version;      /* must be LRAM_ABI_VERSION */
  int32_t backbone;         /* LRAM_BACKBONE_* */
  int32_t d_model;          /* hidden_size / embedding_dim / d_model */
  int32_t n_blocks;         /* n_layer / num_blocks */
  int32_t tokens_per_step;  /* 3: (state, return-to-go, reward), discrete_decision_transformer_model.py:265-275 */
  int32_t pred_token;       /* 1: action is read at the rtg token, tok_to_pred_pos["a"] */
  /* xLSTM */
  int32_t n_heads;          /* mlstm.num_heads == slstm.num_heads (4) */
  int32_t conv_k;           /* conv1d_kernel_size (4) */
  int32_t qkv_blocksize;    /* qkv_proj_blocksize (4) */
  int32_t inner;            /* mLSTM inner dim = ceil64(2 * d_model) */
  int32_t ffn_dim;          /* sLSTM-block gated FFN dim = ceil64(1.3 * d_model) */
  int32_t block_is_slstm[LRAM_MAX_BLOCKS]; /* 1 where the block index is in `slstm_at` */
  int32_t norm_is_rms;      /* 1 when HF config has rms_norm (decision_xlstm.py:190-191) */
  float   ln_eps;           /* 1e-5 */
  /* Mamba */
  int32_t d_inner;          /* expand * d_model */
  int32_t d_state;          /* 16 */
  int32_t d_conv;           /* 4 */
  int32_t dt_rank;          /* ceil(d_model / 16) */
  float   norm_eps;         /* 1e-5 */
  /* token front end / head (multi_domain_discrete_dt_model.py:12-81) */
  int32_t state_dim;        /* 204 (max_state_dim) */
  int32_t act_dim;          /* 8 (max_act_dim) */
  int32_t n_vocab;          /* 274 = discrete_actions + action_channels */
  int32_t n_discrete;       /* 18, also the tokenizer shift */
  int32_t action_channels;  /* 256 */
  float   tok_min;          /* -1 */
  float   tok_max;          /* +1: the bin width is formed in fp32 from the two fp32 bounds, (tok_max - tok_min) / action_channels;
                               for bounds that fp32 does not hold exactly it can differ by an ulp from the reference's double division.
                               De-tokenisation rounds twice, as MinMaxTokenizer.inv_tokenize: fp32(fp32(t * bin_width) + tok_min) */
} lram_config;

typedef struct lram_engine lram_engine; /* opaque */

/* Text of the last error raised on this thread ("" if none). */
const char* lram_last_error(void);

/* ABI version the library was built with. */
int32_t lram_abi_version(void);
/* 64 hex digits: sha256 over the library's sources, headers and compiler flags (lram_amd/build.py::source_hash).  The
 * Python side rebuilds when it differs from the checked-out tree; tests/conftest.py and bench.py assert / report it. */
const char* lram_build_id(void);

/* Create an engine on HIP device `device`.  Replaces the construction of the policy's encoder,
 * xLSTMEncoder.__init__ / MambaEncoder.__init__ (decision_xlstm.py:119-136, decision_mamba.py:52-107). */
int32_t lram_create(const lram_config* cfg, int32_t device, lram_engine** out);

/* Destroy the engine and free all device memory it owns. */
int32_t lram_destroy(lram_engine* e);

/* Upload one weight tensor (host fp32, `numel` elements) under an engine-side name.  Names and shapes
 * are listed by lram_amd/weights.py::engine_layout (derived from the reference checkpoint keys,
 * `policy.state_dict()`, src/algos/decision_transformer_sb3.py:1246-1280).  Replaces load_state_dict. */
int32_t lram_set_weight(lram_engine* e, const char* name, const float* host_data, size_t numel);

/* Check that every weight the configured model needs is present with the right size; resolves the
 * kernel-side pointer tables.  Must be called once after the last lram_set_weight. */
int32_t lram_finalize(lram_engine* e);

/* Allocate (or re-allocate) zeroed recurrent state and activation workspace for `batch` env slots.
 * Replaces `past_key_values = None` / InferenceParams(max_batch_size) (decision_mamba.py:33-38). */
int32_t lram_state_alloc(lram_engine* e, int32_t batch);

/* Bytes of recurrent state held per env slot (the S_env of SURVEY.md 8d). */
int64_t lram_state_bytes_per_env(const lram_engine* e);

/* Zero the recurrent state of the env slots whose mask byte is non-zero (device uint8[batch]); NULL
 * resets every slot.  Replaces `model.past_key_values = None; model.inference_params.reset()`
 * (src/callbacks/evaluation.py:116-119,247-250). */
int32_t lram_reset(lram_engine* e, const uint8_t* dev_env_mask, void* stream);

/* One env-step for all `batch` slots: embed (state, rtg, reward) -> embed_ln -> tokens_per_step
 * recurrent token steps through the block stack -> post norm -> action head -> argmax -> inv_tokenize
 * (with lram_set_sampling armed: -> token drawn from the logits -> inv_tokenize).
 * Replaces policy.forward(..., use_inference_cache=True, past_key_values=...) as called from
 * get_action_pred (src/algos/discrete_decision_transformer_sb3.py:60-68) for every env at once.
 *   dev_obs        device float[batch, state_dim]  (zero-padded obs, decision_xlstm.py:16-19), or, when
 *                  obs_is_embedding != 0, device float[batch, d_model] = embed_image(obs/255) computed by
 *                  the caller (ImpalaCNN stays in PyTorch/MIOpen)
 *   dev_rtg        device float[batch]             returns-to-go (already divided by reward_scale)
 *   dev_reward     device float[batch]             reward token (0 in the reference loop)
 *   dev_reset_mask device uint8[batch] or NULL     slots to reset before this step
 *   discrete       0: continuous head (argmax over n_vocab per action dim, de-tokenised to fp32)
 *                  1: discrete head (argmax over the first n_discrete logits of action dim 0); refused when n_discrete == 0
 *                  LRAM_HEAD_PER_SLOT: the head mode and the action dims in use of every slot come from the slot table
 *                  (lram_set_slot_table); the observation kind stays the call's own
 *   dev_actions    device float[batch, act_dim]    out; discrete: column 0 holds the action index
 *   dev_tokens     device int32[batch, act_dim] or NULL   out; raw token ids
 * Sampling off (the default, a_sample_kwargs = None in the reference): the token is the argmax of its row.  Sampling on
 * (lram_set_sampling): the token is drawn from its row; dev_actions holds what the argmax path would write for that
 * token id (continuous: inv_tokenize(token); discrete: the id), and the call counts as one draw. */
int32_t lram_step(lram_engine* e, const float* dev_obs, int32_t obs_is_embedding, const float* dev_rtg,
                  const float* dev_reward, const uint8_t* dev_reset_mask, int32_t discrete,
                  float* dev_actions, int32_t* dev_tokens, void* stream);

/* Context (re-)prime: `timesteps` consecutive env-steps of stored trajectory data in ONE call, without the action
 * head on the intermediate steps -- the recurrent counterpart of feeding `eval_context_len` timesteps through
 * policy.forward without a cache (src/algos/decision_transformer_sb3.py:628-640,663-666: after
 * `reset_inf_cache_freq` fires the reference re-embeds the context but keeps only the last 3 tokens, SURVEY 3.5 Q5;
 * `chunkwise_step`, decision_xlstm.py:158-159).  Equal to `timesteps` sequential lram_step calls up to
 * fp32 rounding, but processed in chunks: each block's recurrent state is read and written once per chunk.
 * xLSTM with a head dim that is a multiple of 128 (the 16M and 206M geometries): up to 21 timesteps (63 tokens) per
 * chunk through the chunkwise matrix-core kernels (csrc/mlstm_chunk.hip: intra-chunk attention form + one rank-T
 * update of C); otherwise, or with LRAM_PREFILL_CHUNK=0 in the environment at lram_create, 4 timesteps (12 tokens)
 * per chunk through the token-sequential kernels.  The first long prefill grows the activation workspace to 64
 * tokens per env slot (device-synchronising, once).  From two chunks on, three chunks are in flight on engine-owned
 * streams (block i of chunk c + 1 waits for block i of chunk c only): the engine then holds two further copies of that
 * workspace and, for raw observations, the [batch, timesteps, d_model] state embeddings of the context (allocated on the
 * first such call; one chunk at a time if the device has less than 2 GiB to spare, or with LRAM_PREFILL_CHUNK=3).  Results
 * are bit-identical to one chunk at a time and are on `stream` when the call returns.
 *   dev_obs_seq    device float[batch, timesteps, state_dim] (or [batch, timesteps, d_model] embeddings)
 *   dev_rtg_seq, dev_reward_seq   device float[batch, timesteps]
 *   dev_reset_mask applied before the first timestep;  dev_actions (nullable): action at the LAST timestep. */
int32_t lram_prefill(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                     const float* dev_reward_seq, int32_t timesteps, const uint8_t* dev_reset_mask,
                     int32_t discrete, float* dev_actions, int32_t* dev_tokens, void* stream);

/* Score a stored trajectory: lram_prefill with the action head evaluated at EVERY timestep -- the recurrent counterpart of the
 * reference's no-cache forward, which returns action logits at every position, and of the loss it takes from them
 * (src/algos/universal_decision_transformer_sb3.py:398-434: tokenize_actions of the float targets, cross-entropy over
 * act_dim x n_vocab, attention_mask / action_mask).  Per (env, timestep, action dim) it can return the greedy token, its
 * de-tokenised action, the log-probability of a recorded action and the raw logits, without a host round trip per timestep.
 *   inputs, dev_reset_mask, discrete   as lram_prefill (LRAM_HEAD_PER_SLOT included); timesteps >= 1
 *   dev_target_actions   device float[batch, timesteps, act_dim] or NULL: recorded actions, tokenised on the device as
 *                        MinMaxTokenizer.tokenize does (src/tokenizers_custom/minmax_tokenizer.py:14-29):
 *                        trunc((x - tok_min) / bin_width) clamped to 0 .. action_channels - 1, plus n_discrete (fp32 subtract,
 *                        IEEE fp32 division); discrete rows take (int)x
 *   dev_target_tokens    device int32[batch, timesteps, act_dim] or NULL: recorded tokens.  At most one of the two.
 *   dev_valid            device uint8[batch, timesteps] or NULL: 0 masks the OUTPUTS of that (env, timestep) -- the reference's
 *                        attention_mask; every timestep still advances the state
 *   over                 0: logp normalises over all n_vocab logits of the row (the reference's cross-entropy);
 *                        1: over the selectable range -- n_discrete on discrete rows, n_vocab otherwise (what the sampling
 *                        head draws from)
 *   temperature          multiplies the logits, as sample_from_logits does (src/algos/models/model_utils.py:7-32); 1 = the plain
 *                        log-softmax; finite and > 0
 *   dev_actions, dev_tokens, dev_logp   device float / int32 / float [batch, timesteps, act_dim], each nullable
 *   dev_logits           device float[batch, timesteps, act_dim * n_vocab] or NULL
 * logp = temperature * x[target] - logsumexp(temperature * x) with maximum, sum and log in fp64, rounded once to fp32.  A target
 * outside the normalisation range or a non-finite float target gives -inf, a NaN in the range NaN, a -inf logit at the target -inf.
 * Masked timesteps, columns j >= act_dim[slot] of a per-slot call and columns j >= 1 of a discrete = 1 call hold logp 0.0f,
 * token -1, action 0.0f; their logits are not written.
 * At least one output must be given; dev_logp needs a target.  The recurrent state afterwards is what lram_prefill over the
 * same inputs leaves, bit for bit.  Row [b, timesteps - 1] goes through the very head launches lram_prefill makes for its action
 * (and lram_get_taps / lram_score_last then see that row's logits): with sampling off it equals lram_prefill's action bit for
 * bit.  Rows of earlier timesteps take the exact-fp32 matrix-core kernel over the chunk's rows, in blocks of at most 4096 rows
 * through an engine-owned scratch (one region per chunk in flight; LRAM_SCORE_ROWS at lram_create lowers the bound, results do
 * not depend on it).  The call is deterministic: with lram_set_sampling armed it still reports the greedy token, draws nothing
 * and leaves the draw counter alone.  Never captured: in graph mode it runs launch by launch, as long prefills do.
 * Refused (message in lram_last_error, nothing launched, state untouched): mamba_repeat > 1 (lram_set_compat_mode), both
 * targets given, no output given, dev_logp without a target. */
int32_t lram_score(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                   const float* dev_reward_seq, int32_t timesteps, const uint8_t* dev_reset_mask, int32_t discrete,
                   const float* dev_target_actions, const int32_t* dev_target_tokens, const uint8_t* dev_valid, int32_t over,
                   double temperature, float* dev_actions, int32_t* dev_tokens, float* dev_logp, float* dev_logits, void* stream);

/* Stored contexts of PER-ENV length: lram_prefill / lram_score where env b's context has n_b = host_lengths[b] timesteps -- held-out
 * trajectories of different lengths, the demonstrations that prime the envs of an in-context evaluation, the last
 * eval_context_len steps of envs at different points of their episodes (the reference pads such batches and masks them,
 * src/algos/universal_decision_transformer_sb3.py:398-434: attention_mask).  Afterwards every env holds the state of ITS OWN
 * context, so a rollout (lram_step) can follow.
 *   inputs, outputs   laid out exactly as in lram_prefill / lram_score: [batch, timesteps, ...], LEFT-aligned.  Env b's context is
 *                     rows [b, 0 .. n_b); rows [b, n_b .. timesteps) have no influence on any output or state and may hold
 *                     anything, NaN included (the rtg / reward / embedding rows are never read; with raw observations the state
 *                     Linear runs over all rows of dev_obs_seq in one launch and the padded result rows are never read)
 *   host_lengths      HOST int32[batch], each in 0 .. timesteps, handed over as lram_state_copy_slots hands its lists over
 *                     (hipMemcpyAsync from pageable memory, ordered on `stream`, no synchronisation)
 *   n_b == timesteps      the env behaves as in lram_prefill: dev_reset_mask[b] decides whether it continues or restarts
 *   0 < n_b < timesteps   the context REPLACES the slot's state: the slot is reset before its first timestep whatever
 *                         dev_reset_mask[b] says
 *   n_b == 0              the slot is left alone: its state after the call equals its state before it bit for bit (as
 *                         lram_state_export shows it; pending lazy windows are folded first, as by every stored-context call),
 *                         its dev_actions / dev_tokens row holds 0.0f / -1, its score rows are masked.  Such slots still run
 *                         through the kernels on zero tokens: their records are saved into engine-owned scratch
 *                         (count x lram_state_bytes_per_env, allocated on first need) ahead of the first chunk and loaded back
 *                         behind the last
 *   dev_actions / dev_tokens (lram_prefill_ragged)   env b's action at its OWN last timestep n_b - 1
 *   lram_score_ragged   row [b, l], l < n_b, as lram_score writes it (dev_valid and the targets are read at the left-aligned
 *                       row); rows l >= n_b hold logp 0.0f, token -1, action 0.0f on every call, their logits are not written
 * How: the contexts are END-aligned inside the call -- env b starts at call-timestep s_b = timesteps - n_b -- and the chunk plan
 * (lram_context_plan) puts a chunk boundary at every distinct s_b; the env's reset flag is set on that chunk and the token front
 * end feeds it zeros before s_b and its own rows from there on.  No recurrent kernel knows about lengths.  Env b's state
 * afterwards is what lram_prefill of n_b timesteps over its own rows leaves, up to fp32 rounding (the chunk partition differs);
 * chunks of 1-4 timesteps run the token-sequential kernels, longer ones the chunkwise kernels where lram_prefill would.  The lazy
 * matrix memory is materialised first and every chunk of the call runs the materialised kernels.  With every n_b == timesteps
 * the call makes the launches of lram_prefill / lram_score: outputs and state are bit-identical.  Sampling: one draw per
 * lram_prefill_ragged call with dev_actions; lram_score_ragged draws nothing.  Never captured.
 * Cost: chunks <= ceil(timesteps / cap) + distinct starts; with as many distinct lengths as timesteps it degenerates to one
 * timestep per chunk, i.e. towards `timesteps` lram_step calls.
 * Refused (message in lram_last_error, nothing launched, state untouched): whatever lram_prefill / lram_score refuse; a length
 * outside 0 .. timesteps; all lengths 0; tokens_per_step != 3; d_model % 4 != 0; raw observations whose [batch, timesteps,
 * d_model] embeddings exceed 2 GiB; the Mamba modes of lram_set_compat_mode (mamba_repeat > 1; stale_state, where a reset
 * re-initialises layer 0 only and the padding would leak into layers >= 1); scratch for the n_b == 0 slots that would leave less
 * than 2 GiB of device memory free.
 * Stored contexts on a subset of slots without computing the other rows: the context-rows modes of the live prefix
 * (lram_set_context_rows, below; in the default mode kept slots are saved and restored, not skipped, and these entries are
 * refused while slots are parked).  Out of scope: slot lists that are no prefix; the Mamba reference-trajectory
 * modes (contexts from image frames: lram_prefill_frames, below).  The dense entries, the lazy step path and the GEMM dispatcher are unchanged.  (A shorter
 * context that CONTINUES a slot's state is lram_prefill_append / lram_score_append, below.) */
int32_t lram_prefill_ragged(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                            const float* dev_reward_seq, int32_t timesteps, const int32_t* host_lengths,
                            const uint8_t* dev_reset_mask, int32_t discrete, float* dev_actions, int32_t* dev_tokens, void* stream);
int32_t lram_score_ragged(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                          const float* dev_reward_seq, int32_t timesteps, const int32_t* host_lengths,
                          const uint8_t* dev_reset_mask, int32_t discrete, const float* dev_target_actions,
                          const int32_t* dev_target_tokens, const uint8_t* dev_valid, int32_t over, double temperature,
                          float* dev_actions, int32_t* dev_tokens, float* dev_logp, float* dev_logits, void* stream);

/* Stored contexts of per-env length that are APPENDED to the state a slot holds: the ragged entries above, except that a context
 * continues the slot's state instead of replacing it -- an in-context evaluation continued by a demonstration of per-env
 * length, envs at different points of their episodes fed the steps they missed, a trajectory longer than one call can hold
 * scored window by window (window k: lengths clamp(n_b - k W, 0, W), the mask on window 0 only).
 *   inputs, outputs, host_lengths   as in the ragged entries: [batch, timesteps, ...] LEFT-aligned, host int32 lengths in
 *                     0 .. timesteps; rows [b, n_b .. timesteps) are never read (raw observations: the state Linear runs over all
 *                     rows and the padded result rows are never read) and may hold anything, NaN included
 *   n_b > 0           env b's n_b timesteps are appended to the state the slot holds; dev_reset_mask[b] != 0 restarts it before
 *                     its first timestep, whatever n_b is; a NULL mask restarts nobody
 *   n_b == 0          the slot's state afterwards equals its state before the call bit for bit (pending lazy windows are folded
 *                     first, as by every stored-context call); rows [b, *] of the inputs are never read, its dev_actions /
 *                     dev_tokens row holds 0.0f / -1, its score rows are masked.  No record is saved or loaded and no scratch is
 *                     allocated for such slots: there is no "less than 2 GiB free" refusal on these entries
 *   dev_actions / dev_tokens, the score rows, sampling, lazy mode   as the ragged entries
 * How: the chunk plan is the ragged entries' (lram_context_plan).  In every chunk that starts before s_b = timesteps - n_b env b is
 * HELD: the engine hands the state-writing kernels a per-env flag under which they write no byte of the env's recurrent state
 * (matrix memory, normaliser, stabiliser and conv state of an mLSTM block; cell and conv state of an sLSTM block; SSM and conv
 * state of a Mamba layer) and ignore its reset flag; its activation rows are computed on zero tokens and never read.  The flag
 * is a compile-time switch of those kernels: a chunk without a held env -- and every other entry of this header -- launches the
 * instances without it.  With every n_b == timesteps the call makes the launches of lram_prefill / lram_score: outputs and state
 * are bit-identical.  Env b's state afterwards is what n_b lram_step calls from its state before leave, up to fp32 rounding.
 * Refused (message in lram_last_error, nothing launched, state untouched): what the ragged entries refuse, except the scratch
 * rule -- a length outside 0 .. timesteps; all lengths 0; tokens_per_step != 3; d_model % 4 != 0; raw observations whose
 * [batch, timesteps, d_model] embeddings exceed 2 GiB; both Mamba modes of lram_set_compat_mode; parked slots (lram_set_live).
 * Skipping the held envs' rows in the projections (hold stops state writes and, where it is free, state reads) and stored
 * contexts while slots are parked: LRAM_CONTEXT_ROWS_STARTED / _LIVE (lram_set_context_rows, below).  Out of scope: the Mamba
 * reference-trajectory modes.  (Frames: lram_prefill_frames, below.) */
int32_t lram_prefill_append(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                            const float* dev_reward_seq, int32_t timesteps, const int32_t* host_lengths,
                            const uint8_t* dev_reset_mask, int32_t discrete, float* dev_actions, int32_t* dev_tokens, void* stream);
int32_t lram_score_append(lram_engine* e, const float* dev_obs_seq, int32_t obs_is_embedding, const float* dev_rtg_seq,
                          const float* dev_reward_seq, int32_t timesteps, const int32_t* host_lengths,
                          const uint8_t* dev_reset_mask, int32_t discrete, const float* dev_target_actions,
                          const int32_t* dev_target_tokens, const uint8_t* dev_valid, int32_t over, double temperature,
                          float* dev_actions, int32_t* dev_tokens, float* dev_logp, float* dev_logits, void* stream);
/* The chunk plan of such a call, a pure host function (no engine, no GPU): the ascending call-timesteps at which its chunks
 * start.  s_b = timesteps - host_lengths[b]; the plan starts at the smallest s_b over envs with a context (earlier timesteps run
 * no chunk at all), holds every distinct s_b of those envs, and cuts the stretch between two such boundaries (or the last one
 * and `timesteps`) into ceil(len / cap) equal chunks of ceil(len / ceil(len / cap)) timesteps (the last one shorter), cap >= 1
 * being what a dense call of `timesteps` takes per chunk.  Where no env starts inside the call (every context is of full length)
 * the plan is the dense call's own: chunks of `cap` from 0 on.  out_starts receives the starts, *out_n their number; with
 * max_chunks too small nothing is written but *out_n and the call fails.  Errors as the ragged entries' length rules. */
int32_t lram_context_plan(int32_t timesteps, int32_t cap, const int32_t* host_lengths, int32_t batch, int32_t* out_starts,
                          int32_t max_chunks, int32_t* out_n);

/* Log-probabilities of caller-given tokens (device int32[batch, act_dim]: what lram_step* / lram_prefill just returned in
 * dev_tokens) under the logits of the last action-producing call, which are still in the engine's logits buffer: dev_logp
 * (device float[batch, act_dim]) as lram_score defines it, one kernel launch, no draw.  The reference's counterpart is
 * log_softmax(temperature * logits) of the row sample_from_logits drew from (model_utils.py:7-32), gathered at the drawn token;
 * top-k / top-p filtering is NOT applied.  Head mode and slot table are those of that call.  Refused if no action-producing
 * call has happened since lram_state_alloc. */
int32_t lram_score_last(lram_engine* e, const int32_t* dev_tokens, int32_t over, double temperature, float* dev_logp,
                        void* stream);

/* Encoder-only operator: inputs_embeds[batch, tokens, d_model] -> last_hidden_state of the same shape
 * (after post_blocks_norm / norm_f), state advanced by `tokens` (1..4, 6, 9 or 12; any count in 13..64 as well on
 * xLSTM geometries the chunkwise kernels cover, see lram_prefill).  This is the exact plug point of
 * `self.encoder(**encoder_inputs)` (online_decision_transformer_model.py:448). */
int32_t lram_encoder_step(lram_engine* e, const float* dev_inputs_embeds, int32_t tokens,
                          const uint8_t* dev_reset_mask, float* dev_hidden_out, void* stream);

/* Debug/parity taps of the last lram_step: copies into caller device buffers when non-NULL.
 *   dev_tokens_embed float[batch, tokens_per_step, d_model]  embed_ln output (batches of up to 1024 env slots: larger
 *                                                             ones skip the per-step copy this tap costs; pass NULL)
 *   dev_hidden       float[batch, tokens_per_step, d_model]  encoder output (after the final norm)
 *   dev_logits       float[batch, act_dim * n_vocab]         action_net output */
int32_t lram_get_taps(lram_engine* e, float* dev_tokens_embed, float* dev_hidden, float* dev_logits,
                      void* stream);

/* Recurrent-state tensors in the reference's `past_key_values` layout.  `which`:
 *   xLSTM mLSTM block: 0 = C [B,NH,DH,DH]  1 = n [B,NH,DH,1]  2 = m [B,NH,1,1]  3 = conv [B,K,inner]
 *   xLSTM sLSTM block: 0 = slstm_state [4,B,D] (y,c,n,m)      3 = conv [B,K,D]
 *   Mamba layer      : 0 = ssm_state [B,d_inner,d_state]      3 = conv_state [B,d_inner,d_conv]
 * lram_state_numel returns the element count (0 if the tensor does not exist for that block).
 * Invariant checked at import: an sLSTM hidden plane (slstm_state[0] = y) must satisfy |y| < 16 (no NaN) wherever the step runs
 * its recurrent products on binary16 planes of 2^12 y (the default with f16x2 projections; the recurrence itself only produces
 * |y| < 1).  lram_state_import refuses anything else (one reduction + host synchronisation on that tensor); LRAM_SLSTM_SEQ=2 or
 * LRAM_GEMM=f32 select the exact-fp32 recurrence, which has no such limit. */
int64_t lram_state_numel(const lram_engine* e, int32_t block, int32_t which);
int32_t lram_state_export(lram_engine* e, int32_t block, int32_t which, float* dev_dst, void* stream);
int32_t lram_state_import(lram_engine* e, int32_t block, int32_t which, const float* dev_src, void* stream);

/* Capture the kernel sequence of lram_step for the current batch / pointer set into a hipGraph and
 * replay it on later identical calls (launch-latency removal for small batches). enable = 0 disables. */
int32_t lram_set_graph_mode(lram_engine* e, int32_t enable);

/* State representation of the mLSTM matrix memory for lram_step / short lram_encoder_step calls.
 *   mode 0: C_t is materialised -- read and rewritten once per env-step (the reference's representation).
 *   mode 1: lazy -- C_t = g * C_base + sum_j c_j khat_j v_j^T.  A step reads C_base once and appends its tokens to a
 *           window of up to 48 tokens; C_base is rewritten ("folded", fp32 matrix cores) once every `fold_period` steps
 *           per env (0 = keep the current period, default 13; the folds of different envs are staggered).  Same
 *           mathematics as recurrent_step_stabilized_simple ([3P]), ~0.6x the HBM bytes of the
 *           materialised update.  Needs an xLSTM head dim that is a multiple of 128 and at least one mLSTM block: on an
 *           sLSTM-only stack (slstm_at = all) there is no matrix memory, mode 1 is refused with an error, mode 2 stays
 *           materialised at every batch size (lram_get_state_mode = 0) and the automatic slice count stays 1.
 *   mode 2 (default): lazy where one block's matrix memory over the batch is at least 128 MiB (16M: 128 env slots, 206M: 21), else materialised.
 * lram_state_export / import, lram_prefill, hipGraph mode and calls with more than 4 tokens fold every pending window
 * first, so they always see the reference state layout.  LRAM_STATE=eager|lazy|auto (and LRAM_LAZY_PERIOD) in the
 * environment at lram_create set the initial mode.  lram_profile_end in lazy mode: total_ms includes the fold launches,
 * n_launches counts the read passes. */
int32_t lram_set_state_mode(lram_engine* e, int32_t mode, int32_t fold_period);
/* 1 when the lazy representation is in effect for the allocated batch, else 0. */
int32_t lram_get_state_mode(const lram_engine* e);
/* Lazy representation, looked at WITHOUT folding (an export would change the fold schedule of the run it observes): copies
 * for mLSTM block `block`
 *   which 0: the scale g of C_base accumulated since the env's last fold   float[B, NH]
 *   which 1: the stabiliser state m                                         float[B, NH]
 *   which 2: pending window tokens per env (as floats)                       float[B]
 * into dev_dst, as of the last completed step.  Evidence hook of the long-horizon parity tests (the range g and m cover over
 * a 1000-step episode: evaluation.py:130-177 never clears the cache inside an episode); fails in materialised mode. */
int32_t lram_lazy_peek(lram_engine* e, int32_t block, int32_t which, float* dev_dst, void* stream);

/* State of INDIVIDUAL env slots: fork, snapshot / restore, re-pack -- without touching any other slot of the batch.
 * (lram_state_export / lram_state_import move one whole-batch tensor and fold every pending window of every env first; these
 * calls fold nothing.)  The reference's counterpart is indexing the batch axis of `past_key_values`
 * (decision_xlstm.py:138-169) / of InferenceParams.key_value_memory_dict (decision_mamba.py:9-25) for one env.
 *
 * Record: the portable per-env format, lram_slot_state_numel() floats = lram_state_bytes_per_env / 4:
 *   - blocks in order;
 *   - within a block the state tensors that exist, in `which` order 0, 1, 2, 3 (see lram_state_numel above);
 *   - each tensor is the env's slice in the reference layout:
 *       mLSTM block: C [NH, DH, DH], n [NH, DH], m [NH], conv [K, inner]
 *       sLSTM block: slstm_state [4, D] (y, c, n, m), conv [K, D]
 *       Mamba layer: ssm_state [d_inner, d_state], conv_state [d_inner, d_conv]
 *   so a record is exactly the concatenation of env b's slices of what lram_state_export returns.  It does not depend on the
 *   batch size, the state mode or the micro-batch slicing of the engine that wrote it.
 *
 * lram_state_copy_slots: slot host_dst[i] becomes an exact copy of slot host_src[i], as of the last completed step.  Sources may
 *   repeat (fan-out); destinations must be unique, in range and must not be sources (permute by save then load).
 * lram_state_save_slots: dev_records (device float[n, slot_state_numel]) receives the records of the listed slots (in range,
 *   at most `batch` of them; repeats allowed).  Never writes engine state, never changes the fold schedule: in lazy mode the
 *   record's C is g * C_base + sum_j c_j khat_j v_j^T computed on the fly (fp32 FMAs; a slot whose C_base is logically zero
 *   contributes only its window), within the state bar of the folded tensor, not bit-identical to it.
 * lram_state_load_slots: writes the records into the listed slots (unique, in range).  In lazy mode each loaded slot's window is
 *   marked empty (count 0, g = 1).  Where the sLSTM step runs its f16x2 form the hidden planes of the listed records must pass
 *   lram_state_import's rule (|y| < 16, no NaN; one small launch + host synchronisation, before anything is written).
 * Index lists are HOST int32 arrays (validation costs no synchronisation); n = 0 is a no-op.  A refused call (message in
 * lram_last_error) leaves the state as it was.
 *   - Unlisted slots, and the sources of a copy or save, are untouched in both state modes: their state and every later output
 *     are bit-identical to a run without the call.  In lazy mode a copy moves the representation as it is (C_base, window rows,
 *     the live side of coefficients / scale / count word) and folds nothing.
 *   - A copied slot's later trajectory, given its source's inputs: bit-identical in materialised mode; in lazy mode bit-identical
 *     where dst = src modulo the fold period inside one env slice, otherwise equal up to the fp32 rounding of a different
 *     fold schedule (the parity bars of the step).
 *   - Ordering against steps on `stream`: as lram_reset (the launches go to `stream`).  State pointers do not change: a captured
 *     graph stays valid.  With the Mamba stale_state mode every layer is copied all the same.
 *   - NOT moved: slot-table entries (lram_set_slot_table) and the sampling stream -- the Philox counter is keyed by the slot
 *     INDEX, so N slots holding copies of one context draw N independent continuations (best-of-N, branching evaluation).
 *     Per-slot sampling settings (lram_set_sampling_slots) stay with the slot index in the same way: copy / save / load and
 *     lram_reset neither move nor clear them, so the forks of one context can sit on a ladder of temperatures. */
int64_t lram_slot_state_numel(const lram_engine* e);
int32_t lram_state_copy_slots(lram_engine* e, const int32_t* host_src, const int32_t* host_dst, int32_t n, void* stream);
int32_t lram_state_save_slots(lram_engine* e, const int32_t* host_slots, int32_t n, float* dev_records, void* stream);
int32_t lram_state_load_slots(lram_engine* e, const int32_t* host_slots, int32_t n, const float* dev_records, void* stream);

/* Live prefix: step only the env slots that have something to do.
 * The state is allocated for `batch` slots; at any time the first n_live of them are LIVE and slots [n_live, batch) are PARKED.
 * A parked slot keeps its recurrent state and no activation row of it is computed, read or written; what a step still does for
 * it is the lazy matrix memory's bookkeeping (below: a few KB per slot carried to the step's ping-pong side, one fold when its
 * class comes due).  Which env sits
 * in which slot is the caller's business; slots are exchanged with lram_state_swap_slots.  The reference has no counterpart: its
 * batched evaluation keeps forwarding an env that has stopped contributing and throws the result away (evaluation.py:184,
 * 205-212: the `unfinished` mask only gates what is accumulated).
 *
 * lram_set_live: n_live in 1 .. batch.  Cheap: host bookkeeping only, no device synchronisation, no allocation.  Completes a
 *   pending tail fold of the lazy matrix memory on `stream`; drops a captured graph only if n_live changes (n_live is one more
 *   field of the captured step's key).  lram_state_alloc sets n_live = batch, and with n_live == batch every launch, argument and
 *   bit is what it is on an engine that never called the setter.
 * lram_get_live: the current n_live (0: no engine / no state).
 * With n_live < batch:
 *   - lram_step, lram_step_images, lram_step_slots, lram_score_last, lram_score_last_sampled and lram_get_taps read and write rows
 *     < n_live only: every per-slot input, the reset mask included, and every output needs n_live rows; nothing beyond is touched.
 *     The slice, kernel and fusion rules are judged on the live rows, as on an engine allocated with n_live slots; the state
 *     mode (lazy or materialised) was chosen at allocation and does not move.
 *   - lram_step_slots takes the frames of the image slots below n_live, in ascending slot order.
 *   - A step's mask never resets a parked slot; lram_reset takes a `batch`-wide mask and may.
 *   - Sampling: a call is one draw, the counter is engine-wide; a parked slot simply does not draw.
 *   - Lazy matrix memory: folds keep covering every allocated slot of the class that is due until every class has come due once
 *     since the live count changed or a swap / copy moved a window (a parked slot is folded at most once, the host-side bounds
 *     stay true; afterwards every parked window is empty and no fold is launched over them); one small launch per mLSTM block
 *     and step carries the parked slots' bookkeeping over to the step's ping-pong side.  A parked slot's record (lram_state_save_slots) stays within the fold's rounding in C
 *     and bit-identical in every other tensor.
 *   - Refused (message in lram_last_error, nothing launched): lram_prefill, lram_score, their ragged and append forms, lram_encoder_step.
 *     (That is the context-rows mode LRAM_CONTEXT_ROWS_ALL, the default; the other two modes, below, run them on the live prefix.)
 *   - Unchanged, on all `batch` slots: lram_state_export / import, lram_state_copy_slots / save / load / swap, lram_lazy_peek,
 *     lram_reset, lram_set_slot_table, lram_set_sampling_slots.
 *
 * Context rows: which slots the stored-context entries (lram_prefill, lram_score, their ragged, append and frames forms) and
 * lram_encoder_step run on.  lram_set_context_rows is host bookkeeping only: no synchronisation, no allocation; a mode outside
 * 0 .. 2 is refused and the mode stays.  lram_state_alloc sets the mode back to 0.  lram_get_context_rows: the mode (0: no engine).
 *   LRAM_CONTEXT_ROWS_ALL (0)  every allocated slot, refused while slots are parked: launch for launch and bit for bit what the
 *     entries did before the modes existed.
 *   LRAM_CONTEXT_ROWS_LIVE (1)  the live prefix [0, n_live).  The entries read and write rows < n_live only: inputs, host_lengths,
 *     the reset mask and every output have n_live rows; the frames entries take the frames of the image slots below n_live, in
 *     ascending slot order, as lram_step_slots does.  Kernel, slice, chunk-lane and score-scratch rules are judged on the live
 *     rows; the state keeps its allocation and strides; every other refusal of the entries stands (the 2 GiB bound on the state
 *     embeddings is on n_live x timesteps x d_model).  A parked slot's record (lram_state_save_slots) is bit-identical afterwards
 *     in materialised mode; in lazy mode the call folds every slot's pending window first, parked slots included, so a parked
 *     record is bit-identical in every tensor but C, and C stays within the fold's rounding if the slot had a pending window.  With
 *     n_live == batch the launches are mode 0's: bit-identical.  Sampling: one draw per action-producing call, as ever.
 *   LRAM_CONTEXT_ROWS_STARTED (2)  mode 1, and for the entries that take host_lengths (ragged, append, frames with lengths) a row
 *     rule: the lengths must be non-increasing in slot order over the live prefix -- otherwise the call is refused with nothing
 *     launched, the message naming the first slot that breaks the order -- and the chunk that starts at call-timestep t runs rows
 *     [0, r) only, r the number of envs with s_b = timesteps - n_b <= t.  The plan is lram_context_plan's.  No env is ever held,
 *     so every chunk launches the plain kernel instances; no row is computed on zero tokens; a slot of length 0 is never a row,
 *     so nothing is saved to or loaded from scratch and the "less than 2 GiB free" refusal cannot arise.  Resets: a replace call
 *     restarts an env with 0 < n_b < timesteps at its own start, otherwise the caller's mask decides; a mask is used only in the
 *     chunk where the env starts.  Score rows beyond an env's length and the action rows of length-0 slots hold the fill values of
 *     the ragged entries.  Per env, state and outputs equal mode 1's up to fp32 rounding (the projection kernels are chosen by
 *     row count); length-0 and parked slots are bit-identical; with every n_b == timesteps the launches are the dense entry's.
 *     The dense entries and lram_encoder_step behave as in mode 1.
 * lram_context_counts: a measurement aid in the style of lram_image_counts.  out4 receives what happened since the engine was
 *   created or since the last call with reset != 0: stored-context calls, chunks run, env-timesteps computed (the sum over chunks
 *   of rows x timesteps), slot records saved to scratch by the replace entries.  lram_encoder_step is not counted.
 *
 * lram_state_swap_slots: exchanges the recurrent state of slots host_a[i] and host_b[i], live or parked, in ONE launch; folds
 *   nothing and touches no other slot.  Lists as lram_state_copy_slots' (HOST int32); all 2n indices distinct and in range, else
 *   refused with nothing launched.  Lazy mode: the representation moves as it is (C_base, window rows, the live side of
 *   coefficients / scale / count word) and the host-side pending bound of both fold classes is raised to the larger of the two.
 *   After it record[a] is the old record[b] bit for bit, and vice versa.  Slot-table entries, per-slot sampling settings and the
 *   Philox stream stay with the slot INDEX, as for a copy. */
int32_t lram_set_live(lram_engine* e, int32_t n_live, void* stream);
int32_t lram_get_live(const lram_engine* e);
int32_t lram_state_swap_slots(lram_engine* e, const int32_t* host_a, const int32_t* host_b, int32_t n, void* stream);
#define LRAM_CONTEXT_ROWS_ALL     0   /* default: every allocated slot; refused while slots are parked */
#define LRAM_CONTEXT_ROWS_LIVE    1   /* the live prefix [0, n_live) */
#define LRAM_CONTEXT_ROWS_STARTED 2   /* the live prefix, and in every chunk only the envs that have started */
int32_t lram_set_context_rows(lram_engine* e, int32_t mode);
int32_t lram_get_context_rows(const lram_engine* e);
int32_t lram_context_counts(lram_engine* e, int64_t* out4, int32_t reset);

/* Context-window inference: the reference's evaluation with use_inference_cache = False, which is its default and what its shipped
 * configs run (src/algos/decision_transformer_sb3.py:86).  At every env-step the model is run FROM AN EMPTY STATE over the env's
 * last K = eval_context_len timesteps, left-padded to K (predict / pad_inputs, decision_transformer_sb3.py:621-691) -- with the true
 * rewards of past timesteps, and with the bookkeeping of the evaluation loop (src/callbacks/evaluation.py:130-251): the reward of
 * the last step patched in, a finished episode's returns-to-go rewritten to the returns obtained, the context pruned to the last
 * episodes.  The engine keeps the last K timesteps of every env slot in a device ring; one entry is the state-token embedding
 * (d_model floats, before embed_ln), the return-to-go and the reward.  How many entries count is n_b in 0 .. K per slot, and every
 * slot has its own ring position; both are kept on the host and go to the device with the call, nothing is read back.  A window
 * step costs a K-timestep lram_prefill over the rows it runs plus two passes over rows x K x d_model floats.
 *
 * lram_window_alloc   allocates the ring for K = timesteps >= 1 (all n_b = 0, no pad entry; about 2 x batch x K x d_model floats);
 *                     0 frees it; lram_state_alloc frees it too.  Synchronises the device.  Refused: state not allocated,
 *                     tokens_per_step != 3, d_model % 4 != 0, [batch, K, d_model] beyond 2 GiB.
 * lram_window_set_pad the pad entry of LRAM_WINDOW_PAD_REFERENCE: dev_pad_obs float[state_dim] through the state Linear, or
 *                     float[d_model] taken as it is (obs_is_embedding).  What the reference's zero padding becomes once it is
 *                     normalised and embedded.  It belongs to the ring: lram_window_alloc drops it.
 * lram_window_set_slots / lram_window_get_slots   which slots a window step runs.  LRAM_WINDOW_SLOTS_SHARED (the default;
 *                     lram_window_alloc and lram_state_alloc set it back): every slot, and parked slots are refused.
 *                     LRAM_WINDOW_SLOTS_OWN: the live prefix [0, n_live) of lram_set_live -- see "live rows" below.  Host bookkeeping
 *                     only: no synchronisation, no allocation, the ring is not touched.  Refused: no ring, a mode other than 0 or 1.
 * lram_step_window    for every env slot b the call runs, in this order:
 *     1 reset    host_reset[b] != 0: n_b = 0, dev_prev_reward[b] is ignored
 *     2 patch    otherwise, if n_b > 0: the newest entry's reward = dev_prev_reward[b] (it was pushed with reward 0)
 *     3 relabel  host_relabel[b] = m > 0: the rtg of the newest min(m, n_b) entries = the fp32 suffix sum of those entries'
 *                rewards as they stand after the patch, accumulated from the newest backwards (s = r_newest, then s = r_j + s):
 *                discount_cumsum with gamma 1
 *     4 keep     host_keep[b] = k > 0: n_b = min(n_b, k), after the relabel
 *     5 push     (embed_state(dev_obs[b]) or dev_obs[b] itself, dev_rtg[b], 0) is appended, n_b = min(n_b + 1, K): the oldest
 *                entry falls out.  Raw observations go through the state Linear at the call's rows
 *     6 the windows, oldest to newest, go through the stored-context body from an empty state for every slot, and dev_actions /
 *       dev_tokens (the latter nullable) take the action of the last timestep.  pad_mode LRAM_WINDOW_PAD_REFERENCE: the rows ahead of a
 *       slot's n_b hold (pad entry, rtg 0, reward 0) and the call makes the launches of lram_prefill over K timesteps of
 *       embeddings with every slot reset -- outputs, logits (lram_get_taps) and state are bit-identical to that call.
 *       LRAM_WINDOW_PAD_NONE: only the n_b real timesteps count; the launches are those of lram_prefill_ragged with lengths n_b
 *       (one chunk boundary per distinct length).
 *   dev_obs          device float[batch, state_dim] (or [batch, d_model] embeddings)
 *   dev_rtg, dev_prev_reward   device float[batch]
 *   host_reset (uint8), host_relabel, host_keep (int32)   HOST arrays [batch], each nullable (nobody reset / relabelled / pruned)
 *   The recurrent state afterwards is what that stored-context call leaves: a window step and lram_step on one engine overwrite
 *   each other's state.  Sampling: one draw per call, as lram_prefill with dev_actions.  Never captured.
 *   Live rows (LRAM_WINDOW_SLOTS_OWN with n_live < batch, the convention of lram_step): dev_obs, dev_rtg, dev_prev_reward and the
 *   host arrays have n_live rows, dev_actions / dev_tokens take n_live rows, and steps 1 - 6 run on slots [0, n_live) alone: the
 *   stored-context body as under LRAM_CONTEXT_ROWS_LIVE (outputs, logits and state bit-identical to lram_prefill[_ragged] in that
 *   mode over the live slots' windows; lram_context_counts grows by n_live x K env-timesteps in pad mode 0).  A parked slot's ring
 *   rows, position, count and recurrent state are untouched bit for bit, and no row of it is computed.  With every slot live the
 *   two modes make the same launches.
 *   Refused (message in lram_last_error, nothing launched, ring, counts and state untouched): no ring; pad mode 0 without a pad
 *   entry; a pad mode other than 0 or 1; parked slots (lram_set_live) in LRAM_WINDOW_SLOTS_SHARED; a context-rows mode other than
 *   LRAM_CONTEXT_ROWS_ALL set by the caller (in either slots mode); both
 *   Mamba modes of lram_set_compat_mode; a relabel on a reset slot; a negative relabel or keep; a NULL dev_obs, dev_rtg,
 *   dev_prev_reward or dev_actions; whatever lram_prefill refuses for `discrete`.
 *   That promise covers the refusals, which are all made before the first launch.  A call that fails LATER -- device memory running
 *   out while the stored-context body grows its workspace or the tables of a call of per-env lengths -- has already done steps
 *   1 - 5: the ring, its counts and the positions of the call's slots are advanced by one timestep, consistently on host and device
 *   (lram_window_peek shows them), and no action was produced.
 * lram_window_peek    copies the windows, END-aligned and oldest to newest with zeros in the rows ahead of n_b, into dev_emb
 *                     float[batch, K, d_model], dev_rtg and dev_reward float[batch, K], and the counts into host_counts
 *                     int32[batch]; every pointer is nullable.  All `batch` slots, live or parked, in either slots mode.
 *
 * Windows move with their slots, beside the state movers and by their host-list rules (lram_state_copy_slots / _swap_slots /
 * _save_slots / _load_slots); one launch each, in both slots modes, on live or parked slots.  They move whole windows -- entries,
 * count and position -- touch no other slot and no recurrent state; the state movers keep leaving the ring alone.
 * lram_window_copy_slots   slot host_dst[i]'s window becomes slot host_src[i]'s.  Sources may repeat (fan-out); destinations are
 *                     unique and no slot is both source and destination.
 * lram_window_swap_slots   exchanges the windows of slots host_a[i] and host_b[i]; all 2n indices distinct.
 * lram_window_slot_numel   floats in one record: K x (d_model + 2) + 1 (0 and a message in lram_last_error without a ring).
 * lram_window_save_slots   record i (dev_records float[n, numel]) = slot host_slots[i]'s window as lram_window_peek lays it out:
 *                     K x d_model embeddings, K rtg, K rewards, END-aligned and oldest to newest with zeros ahead of n_b, then n_b
 *                     as one trailing float.  Position-free: a record loads into any engine with the same K and d_model, whatever
 *                     its ring positions.  Slots may repeat; at most `batch` per call.
 * lram_window_load_slots   the inverse, slots unique.  The counts reach the host through one read-back of n floats, which
 *                     synchronises `stream` (the only window call besides lram_window_alloc that waits for the device); a record
 *                     whose trailing float is no integer in 0 .. K is refused before anything is written.
 * Refused, with ring, counts, positions and state untouched: no ring, an index out of range, a destination listed twice, a slot
 * that is both source and destination, (swap, load) a slot listed twice, a NULL list or records with n > 0.  n = 0 is a no-op.
 * Out of scope: slot tables in window mode, reading the ring in place from the chunk front end. */
#define LRAM_WINDOW_PAD_REFERENCE 0   /* pad entry, rtg 0, reward 0 ahead of a shorter window: the reference's pad_inputs */
#define LRAM_WINDOW_PAD_NONE      1   /* only the real timesteps count */
#define LRAM_WINDOW_SLOTS_SHARED  0   /* a window step runs every slot; parked slots are refused */
#define LRAM_WINDOW_SLOTS_OWN     1   /* a window step runs the live prefix; parked slots keep their windows */
int32_t lram_window_alloc(lram_engine* e, int32_t timesteps);
int32_t lram_window_set_pad(lram_engine* e, const float* dev_pad_obs, int32_t obs_is_embedding, void* stream);
int32_t lram_step_window(lram_engine* e, const float* dev_obs, int32_t obs_is_embedding, const float* dev_rtg,
                         const float* dev_prev_reward, const uint8_t* host_reset, const int32_t* host_relabel,
                         const int32_t* host_keep, int32_t pad_mode, int32_t discrete, float* dev_actions, int32_t* dev_tokens,
                         void* stream);
int32_t lram_window_peek(lram_engine* e, float* dev_emb, float* dev_rtg, float* dev_reward, int32_t* host_counts, void* stream);
int32_t lram_window_set_slots(lram_engine* e, int32_t mode);
int32_t lram_window_get_slots(const lram_engine* e);
int32_t lram_window_copy_slots(lram_engine* e, const int32_t* host_src, const int32_t* host_dst, int32_t n, void* stream);
int32_t lram_window_swap_slots(lram_engine* e, const int32_t* host_a, const int32_t* host_b, int32_t n, void* stream);
int64_t lram_window_slot_numel(const lram_engine* e);
int32_t lram_window_save_slots(lram_engine* e, const int32_t* host_slots, int32_t n, float* dev_records, void* stream);
int32_t lram_window_load_slots(lram_engine* e, const int32_t* host_slots, int32_t n, const float* dev_records, void* stream);

/* Micro-batch pipeline (xLSTM): the env slots are processed as `n` slices on engine-owned HIP streams; the
 * HBM-bound matrix-memory kernels of all slices run back to back on one stream while the other slices'
 * fp32-MFMA projections overlap them.  n = 1 disables it, 0 = automatic (2 slices where one mLSTM block's matrix memory over the batch reaches 512 MiB -- 16M from 512 env slots,
 * 206M from 82 -- and for Mamba from 1024 env slots), max 8.
 * Results do not depend on n (envs are independent). */
int32_t lram_set_micro_batches(lram_engine* e, int32_t n);

/* Reference-trajectory modes of the Mamba agent (Mamba engines only; defaults 1 / 0 = one state advance per
 * env-step, a reset empties every layer).
 *   mamba_repeat R > 1: DiscreteDecisionMamba.get_action_pred (src/algos/decision_mamba.py:107-122) calls the policy
 *     once per action dim with the inference cache on, so the conv / ssm state advances R = env_act_dim times per
 *     env-step on the same (state, rtg, reward) tokens and action dim i is the prediction of forward i.  lram_step
 *     then runs R forwards (reset mask applied before the first); columns >= R hold forward R - 1.  Discrete heads
 *     (act_dim 1 in the reference) always take one forward.
 *   stale_state != 0: InferenceParams.reset() (src/algos/decision_mamba.py:20-25) only zeroes seqlen_offset, and
 *     MambaEncoder.forward bumps it inside the layer loop (src/algos/models/decision_mamba.py:130-149): layer 0 runs
 *     its full scan from an empty state, layers >= 1 step on from the previous episode's cache.  The reset mask of
 *     lram_step / lram_prefill and lram_reset then re-initialise layer 0 only. */
int32_t lram_set_compat_mode(lram_engine* e, int32_t mamba_repeat, int32_t stale_state);
int32_t lram_get_compat_mode(const lram_engine* e, int32_t* mamba_repeat, int32_t* stale_state);

/* Sampling mode of the action head, off by default: the counterpart of the agents' `a_sample_kwargs`
 * (src/algos/discrete_decision_transformer_sb3.py:8-11,63-64; src/algos/decision_mamba.py:118-120), which hand the head's
 * logits to sample_from_logits(logits, temperature, top_k, top_p) (src/algos/models/model_utils.py:7-32).  With enable != 0
 * lram_step, lram_step_images and lram_prefill draw each (env, action dim) token from its row of logits -- n_vocab values, or
 * the first n_discrete of action dim 0 for the discrete head -- instead of taking the argmax.  Row by row, as the reference:
 *   1. top_p > 0: q = torch.quantile(row, top_p) in float64 (linear interpolation between the order statistics at
 *      floor / ceil(top_p * (n - 1))); unless q equals the row's maximum, every logit <= q is dropped.  This is a quantile of
 *      the logit VALUES, not nucleus sampling.
 *   2. top_k > 0: only the k largest of what is left stay (ties at the k-th place: the lowest index first).
 *   3. probabilities = softmax(temperature * logits) over what is left: `temperature` MULTIPLIES the logits, as in the
 *      reference (a larger value sharpens the distribution).
 *   4. the token is the first one, in vocabulary order, whose cumulative probability exceeds one uniform u in [0, 1).
 * The reference draws with torch's generator; here u is word x0 of Philox4x32-10 (Salmon et al., SC'11), u = x0 * 2^-32, with
 *      key     = (seed & 0xffffffff, seed >> 32)
 *      counter = ((slot_base + s) & 0xffffffff, j, d & 0xffffffff, d >> 32)
 * for env slot s (index within this engine), action dim j and draw d.  d counts the action-producing calls (lram_step,
 * lram_step_images, lram_prefill with dev_actions) since sampling was last armed: one per call, also when the Mamba
 * reference-trajectory mode runs several forwards in it (they share d and differ in j).  Resets do not touch d.  It lives in
 * device memory and is advanced on the device behind the head launches of the call, so replayed hipGraph steps draw afresh.
 * slot_base is the global index of this engine's first env slot: engines holding ranges of one slot numbering (lram_amd.dist
 * shard bounds) draw what one engine over all slots would.
 * Rows the rule has no answer for -- a NaN in the row, a maximum of +inf or -inf, or nothing left after step 1 (a NaN
 * quantile) -- take the argmax rule of the default path (the reference raises); -inf logits have probability 0.
 * Errors: temperature not finite or <= 0, top_p outside [0, 1], top_k < 0 or > n_vocab, n_vocab > 512; a discrete-head call
 * with top_k > n_discrete fails at that call.  enable = 0 restores the argmax launches; the other arguments are then ignored.
 * Arming zeroes d.  Synchronises the device and drops a captured graph: not a hot-path call. */
int32_t lram_set_sampling(lram_engine* e, int32_t enable, double temperature, int32_t top_k, double top_p, uint64_t seed,
                          uint64_t slot_base);
/* Reads the settings back (the last armed ones when disabled) and, into *draws, d (0 when disabled; synchronises the device).
 * Any pointer may be NULL. */
int32_t lram_get_sampling(lram_engine* e, int32_t* enable, double* temperature, int32_t* top_k, double* top_p, uint64_t* seed,
                          uint64_t* slot_base, uint64_t* draws);

/* Per-slot sampling settings: host arrays of length `batch`, entry b for env slot b -- mode (0 = greedy: the argmax rule of the
 * default path, bit for bit; 1 = sample), temperature, top_k, top_p with the meaning they have in lram_set_sampling.  While a
 * table is set every row of every action-producing call takes its slot's entry in place of lram_set_sampling's temperature /
 * top_k / top_p; seed, slot_base and the draw counter d stay those of lram_set_sampling, and d advances once per call as before
 * (greedy slots read no uniform).  All four pointers NULL clears the table: the launches are then again exactly those of
 * lram_set_sampling alone (the per-slot table is a separate kernel instantiation).
 * Needs sampling armed; lram_set_sampling (arming or disarming) and lram_state_alloc clear the table.  Errors, each naming the
 * slot: mode > 1, temperature not finite or <= 0, top_p outside [0, 1], top_k < 0 or > n_vocab.  The top_k bound of the head
 * in use is per slot: a call whose head (its `discrete` argument, or the slot table's flag under LRAM_HEAD_PER_SLOT /
 * lram_step_slots) gives some SAMPLING slot n_discrete < top_k logits is refused before anything is launched, with a text
 * naming the slot; greedy slots and continuous slots of a mixed table are not bound by n_discrete.
 * Synchronises the device and drops a captured graph: not a hot-path call. */
int32_t lram_set_sampling_slots(lram_engine* e, const uint8_t* mode, const double* temperature, const int32_t* top_k,
                                const double* top_p);
/* Copies the table in effect back (host arrays of length batch; any pointer may be NULL); *set = 0 and nothing written when
 * no table is set. */
int32_t lram_get_sampling_slots(lram_engine* e, uint8_t* mode, double* temperature, int32_t* top_k, double* top_p, int32_t* set);

/* Log-probabilities [batch, act_dim] of dev_tokens [batch, act_dim] under the distribution the sampling head draws from: the
 * logits of the last action-producing call, the settings armed NOW (the per-slot entries where a table is set, those of
 * lram_set_sampling otherwise), steps 1-3 of lram_set_sampling applied -- t * (x_tok - max) - log(sum over the support of
 * exp(t * (x - max))) in fp64, one fp32 rounding at the store.  A token outside the support or outside 0 .. n - 1: -inf; a
 * support of one entry: exactly 0; a row on the argmax rule (a greedy slot, a NaN, a maximum of +-inf, nothing left): 0 at the
 * argmax token, -inf elsewhere; columns the slot does not use and token -1: the fill value 0 (as lram_score_last).
 * Deterministic: draws nothing, d is unchanged.  Errors as lram_score_last when there are no logits yet; sampling not armed
 * is an error too. */
int32_t lram_score_last_sampled(lram_engine* e, const int32_t* dev_tokens, float* dev_logp, void* stream);

/* Per-kernel timing of the recurrent step, measured with HIP events on the stream the kernels are
 * launched on.  lram_profile_begin arms it; every later lram_step records one (start, stop) event pair
 * around the mLSTM cell-update launches (xLSTM) or the selective-state-update launches (Mamba).
 * lram_profile_end synchronises and returns total milliseconds and number of launches timed. */
int32_t lram_profile_begin(lram_engine* e);
/* The same, timing only every n-th lram_step (the first one after this call included): each timed launch is bracketed by two
 * event packets on the state-pass queue, and at 21 launches per step that bookkeeping costs the headline 1.3-1.8 % when every
 * step carries it (profiles/r05_ab_kernel_timing.txt).  lram_profile_end* report the sampled launches only. */
int32_t lram_profile_begin_sampled(lram_engine* e, int32_t every_n_steps);
int32_t lram_profile_end(lram_engine* e, double* total_ms, int64_t* n_launches);
/* The same, with the lazy mode's fold launches (timed on their own stream) reported apart from the state-pass
 * launches, so that each figure can be held against the per-kernel averages of a rocprofv3 --kernel-trace run. */
int32_t lram_profile_end_split(lram_engine* e, double* main_ms, int64_t* n_main, double* aux_ms, int64_t* n_aux);

/* Measurement aid: how many projection launches each kernel family of the dispatcher (engine.hip::gemm) has served since
 * lram_create or the last call with `reset` != 0 -- out[0] f16x2, out[1] bf16x3, out[2] exact fp32 MFMA (tile / GEMV),
 * out[3] few-row fp32 kernel, and out[4..7] the fp32-equivalent FLOPs (2 M N K, summed) of the same four.  bench.py labels
 * its workload line from these instead of from the LRAM_GEMM environment variable.  (The reference has no counterpart:
 * nn.Linear calls at src/algos/models/decision_mamba.py:78-93 / [3P] xlstm proj_up / proj_down go to the vendor BLAS.) */
int32_t lram_gemm_counts(lram_engine* e, double* out8, int32_t reset);

/* Measurement aid: which form of the sLSTM recurrence (engine_xlstm.hip::slstm_block) the engine has launched since lram_create
 * or the last call with `reset` != 0 -- out[0] token-kernel launches (one per token and slice), out[1] step-kernel launches (one
 * per pass and slice), out[2] launches of the pointwise kernel behind a recurrent GEMM (one per token and slice).  The choice
 * depends on d_model / num_heads, the slice size and LRAM_SLSTM_FUSED_ROWS / LRAM_SLSTM_SEQ; tests assert the form they mean
 * to compare really ran.  (Reference: one sLSTMLayer.step per token, src/algos/models/decision_xlstm.py:155-166.) */
int32_t lram_slstm_counts(lram_engine* e, int64_t* out3, int32_t reset);

/* Measurement aid: what the frame-list front end (lram_embed_frames, lram_prefill_frames, lram_score_frames) has done since
 * lram_create or the last call with `reset` != 0 -- out[0] frames convolved, out[1] tiles launched (one pass of the conv stages
 * each), out[2] launches of the CNN's Linear.  The env-step entries (lram_embed_images, lram_step_images, lram_step_slots) are
 * not counted.  Tests read it to prove that padded frames were skipped. */
int32_t lram_image_counts(lram_engine* e, int64_t* out3, int32_t reset);

/* Standalone kernel entry points used by tests and micro-benchmarks. */
/* C[M,N] = A[M,K] * W[N,K]^T (+ bias[N]) (+ residual C_in)   fp32, MFMA 32x32x2 f32 (exact k-ordered fma chain) */
int32_t lram_gemm_f32(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c,
                      int64_t ldc, const float* dev_bias, int32_t accumulate, int32_t m, int32_t n,
                      int32_t k, void* stream);
/* Same contract through the bf16x3 kernel the engine uses for its projections (each fp32 operand split into
 * three bf16 pieces, six bf16 MFMA products accumulated in fp32: fp32-level accuracy, not bit-identical to
 * lram_gemm_f32).  W must be contiguous [n, k], k a multiple of 8.  Splits W into a temporary and synchronises
 * the stream: test / micro-benchmark entry, not a hot-path call. */
int32_t lram_gemm_bf16x3(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c,
                         int64_t ldc, const float* dev_bias, int32_t accumulate, int32_t m, int32_t n,
                         int32_t k, void* stream);
/* Same contract through the few-row kernel (gemm_f32.hip::gemm_skinny_kernel: one 32 x 32 tile of the exact fp32 matrix
 * instruction per workgroup, K split over the waves, operands straight into registers; the engine takes it for GEMMs of
 * 9 .. 384 operand rows and K <= 1024).  k >= 32, k / lda / ldw multiples of 4, 16-byte aligned operands.  Test entry. */
int32_t lram_gemm_skinny(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c,
                         int64_t ldc, const float* dev_bias, int32_t accumulate, int32_t m, int32_t n,
                         int32_t k, void* stream);
/* Same contract through the narrow-output kernel (gemm_narrow.hip: 16 rows x all n <= 96 columns per workgroup, exact fp32 matrix
 * instruction, A staged coalesced through LDS, W packed in fragment order; the engine takes it for Mamba's x_proj --
 * mamba_ssm.Mamba.x_proj, reached from src/algos/models/decision_mamba.py:130-147 -- from 256 operand rows).  W contiguous
 * [n, k], k a multiple of 64 and >= 256, lda a multiple of 4, accumulate must be 0.  Packs W into a temporary and synchronises
 * the stream: test / micro-benchmark entry. */
int32_t lram_gemm_narrow(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c,
                         int64_t ldc, const float* dev_bias, int32_t accumulate, int32_t m, int32_t n,
                         int32_t k, void* stream);
/* The same kernel family with the products formed as in lram_gemm_f16x2 (rows scaled by a power of two, two binary16 pieces per
 * operand, hi*hi + hi*lo + lo*hi on the f16 matrix instruction, exact un-scaling): the form the engine runs for x_proj wherever
 * its projections run as f16x2 and the conv kernel hands the operand's row maxima over.  Same argument rules as lram_gemm_narrow;
 * splits W and takes A's row maxima in temporaries, synchronises the stream: test / micro-benchmark entry. */
int32_t lram_gemm_narrow_f16x2(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c,
                               int64_t ldc, const float* dev_bias, int32_t accumulate, int32_t m, int32_t n,
                               int32_t k, void* stream);
/* Same contract through the f16x2 kernel (each fp32 operand row scaled by a power of two and split into two binary16
 * pieces, three f16 MFMA products accumulated in fp32, exact un-scaling: fp32-level accuracy at half the matrix-core
 * work of bf16x3; gemm_f16x2.hip).  Splits W and computes A's row scales into temporaries, synchronises the stream:
 * test / micro-benchmark entry. */
int32_t lram_gemm_f16x2(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c,
                        int64_t ldc, const float* dev_bias, int32_t accumulate, int32_t m, int32_t n,
                        int32_t k, void* stream);
/* The f16x2 arithmetic with the activation operand pre-split too (gemm_f16x2p.hip): A goes through the row-split kernel
 * (two f16 planes of the row-scaled rows + inverse scales -- what the engine's norm kernels write directly), both operands
 * are then staged global -> LDS by DMA and the inner loop is MFMAs only.  k a multiple of 32, <= 3072.  Same accuracy
 * contract as lram_gemm_f16x2 (the pieces and the products are the same; the result is bit-identical to it).
 * Test / micro-benchmark entry. */
int32_t lram_gemm_f16x2_presplit(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c,
                                 int64_t ldc, const float* dev_bias, int32_t accumulate, int32_t m, int32_t n,
                                 int32_t k, void* stream);
/* The same operands through the 8-phase 256 x 256 kernel (gemm_f16x2_8p.hip), which the pre-split launcher picks by itself
 * only for large launches: same argument rules, bit-identical result.  Test / micro-benchmark entry. */
int32_t lram_gemm_f16x2_presplit_8p(const float* dev_a, int64_t lda, const float* dev_w, int64_t ldw, float* dev_c,
                                    int64_t ldc, const float* dev_bias, int32_t accumulate, int32_t m, int32_t n,
                                    int32_t k, void* stream);
/* The device code of the sampling head on caller data (test / evidence entry): row r = dev_logits + r * ld holds n <= 512
 * logits (ld = 0: every row is row 0), dev_uniform[r] (device double) its uniform in [0, 1); dev_tokens[r] (device int32)
 * receives the token of steps 1-4 of lram_set_sampling. */
int32_t lram_sample_tokens(const float* dev_logits, int64_t rows, int32_t n, int64_t ld, double temperature, int32_t top_k,
                           double top_p, const double* dev_uniform, int32_t* dev_tokens, void* stream);
/* The same with per-row settings (test / evidence entry of lram_set_sampling_slots / lram_score_last_sampled): dev_mode uint8,
 * dev_temperature double, dev_top_k int32, dev_top_p double, each [rows] on the device.  dev_uniform + dev_tokens_out
 * (both or neither): the drawn token per row.  dev_tokens_in + dev_logp_out (both or neither): the log-probability of the
 * given token per row under that row's settings (token -1: 0).  At least one pair must be given. */
int32_t lram_sample_rows(const float* dev_logits, int64_t rows, int32_t n, int64_t ld, const uint8_t* dev_mode,
                         const double* dev_temperature, const int32_t* dev_top_k, const double* dev_top_p,
                         const double* dev_uniform, const int32_t* dev_tokens_in, int32_t* dev_tokens_out, float* dev_logp_out,
                         void* stream);
/* The uniforms an armed step would use at draw `draw`: dev_out (device double[n_slots, act_dim]) [s, j] for env slots
 * slot_base .. slot_base + n_slots - 1 (test / evidence entry). */
int32_t lram_sample_uniforms(uint64_t seed, uint64_t slot_base, int64_t n_slots, int32_t act_dim, uint64_t draw,
                             double* dev_out, void* stream);
/* The device code of the scoring head on caller logits (test / evidence entry, as lram_sample_tokens is for the sampling head):
 * dev_logits device float[rows, act_dim * n_vocab]; targets, dev_valid (uint8[rows]) and outputs ([rows, act_dim]) as in
 * lram_score; discrete 0 or 1. */
int32_t lram_score_tokens(const float* dev_logits, int64_t rows, int32_t act_dim, int32_t n_vocab, int32_t n_discrete,
                          int32_t action_channels, float tok_min, float tok_max, int32_t discrete, const float* dev_target_actions,
                          const int32_t* dev_target_tokens, const uint8_t* dev_valid, int32_t over, double temperature,
                          float* dev_actions, int32_t* dev_tokens, float* dev_logp, void* stream);
/* Image observations: uint8 frames [batch, channels, height, width] -> state-token embeddings [batch, d_model]
 * through the IMPALA CNN (3 x [conv3x3 -> maxpool(3,2,1) -> 2 residual blocks], 16/32/32 channels, ReLU, flatten,
 * Linear, ReLU).  Replaces `self.embed_image(state.float() / 255)` (online_decision_transformer_model.py:523-526;
 * module src/algos/models/image_encoders.py:10-131, built at multi_domain_discrete_dt_model.py:43-46).  Needs the
 * `embed_image.*` tensors (reference names) uploaded before lram_finalize; the result is passed to lram_step /
 * lram_prefill with obs_is_embedding = 1.  Any height, width >= 1 are accepted, square or not, provided the size after the
 * three poolings (each extent (n - 1) / 2 + 1) matches embed_image.linear.0.weight, and the size may change between calls
 * (so may it in lram_step_images and lram_step_slots); any other size is an error that names it. */
int32_t lram_embed_images(lram_engine* e, const uint8_t* dev_images, int32_t channels, int32_t height, int32_t width,
                          float* dev_embeddings, void* stream);
/* One env-step from image observations: lram_embed_images + lram_step(obs_is_embedding = 1) as ONE call -- what the reference's
 * forward does with image states (`compute_inputs`: `state_embeddings = self.embed_image(states / 255)` then the token stack,
 * online_decision_transformer_model.py:463-530).  Same results as the two calls; the engine runs the CNN per env slice on the
 * slice's own stream and starts the step's state-pass work that does not depend on the observation (the lazy matrix memory's
 * folds) beside it.  Frames uint8 [batch, channels, height, width]; other arguments as lram_step. */
int32_t lram_step_images(lram_engine* e, const uint8_t* dev_images, int32_t channels, int32_t height, int32_t width,
                         const float* dev_rtg, const float* dev_reward, const uint8_t* dev_reset_mask, int32_t discrete,
                         float* dev_actions_out, int32_t* dev_tokens_out, void* stream);
/* ANY number of frames, uint8 [n_frames, channels, height, width] -> [n_frames, d_model], n_frames >= 1 whatever the batch:
 * lram_embed_images' arithmetic through the frame-list path of the stored contexts below.  The frames go through the conv
 * stages in tiles of LRAM_IMG_TILE frames (read at lram_create; capped so that one tile's maps stay within 2 GiB), every
 * tile's last map into its rows of one [n_frames, features] operand, and ONE Linear runs over all of it: the result does not
 * depend on the tile, bit for bit.  (It may differ in the last bits from lram_embed_images on the same frames: the Linear's
 * kernel is chosen by row count.)  Refused when that operand would exceed 2 GiB. */
int32_t lram_embed_frames(lram_engine* e, const uint8_t* dev_frames, int64_t n_frames, int32_t channels, int32_t height,
                          int32_t width, float* dev_embeddings, void* stream);
/* Stored contexts whose observations are uint8 frames: lram_prefill / lram_score (host_lengths NULL), their ragged forms
 * (host_lengths given, append 0: the replace rule) and their append forms (append 1), with the IMPALA CNN as the source of the
 * state embeddings -- what the reference's forward does with a batch of image trajectories (`compute_inputs`,
 * online_decision_transformer_model.py:463-530, under the masked loss of universal_decision_transformer_sb3.py:398-434).
 *   dev_frames        uint8 [n, timesteps, channels, height, width], LEFT-aligned like every other input.  Without a slot table
 *                     n = batch.  With one, n = its image slots, in ascending slot order (as lram_step_slots takes frames).
 *   dev_obs_seq       float [batch, timesteps, state_dim]: required when a slot table with vector slots is set -- the state Linear
 *                     runs over all of its rows first and the image slots' rows are then overwritten, so whatever the rows of
 *                     image slots hold, NaN included, reaches no output.  Never read otherwise (NULL is fine).
 *   host_lengths      NULL: every context has all `timesteps`.  Else as in the ragged / append entries, and only frames [b, l] with
 *                     l < n_b are read: the engine builds, on the device, a list of the frames that count ({frame index, row
 *                     b * timesteps + l} per entry, from the per-env starts and the slot table's image list) and the CNN runs
 *                     over that list alone -- a padded frame is never read or convolved and costs nothing.
 *   append            0 or 1; ignored without host_lengths.
 *   everything else   as in lram_prefill / lram_score and their ragged / append forms: one body, the same refusals in the same order.
 * With every length equal to `timesteps` the call makes the dense call's launches.  State, actions, tokens and log-probabilities
 * are bit-identical to lram_prefill / lram_score(obs_is_embedding = 1) over lram_embed_frames of the same frames where the
 * list is the same (a dense call); per-env lengths shorten the list, and the Linear's kernel follows its row count.
 * Refused in addition (nothing launched, state untouched): no embed_image.* weights; a frame size that does not fit the Linear;
 * tokens_per_step != 3, d_model % 4 != 0 or a Mamba mode of lram_set_compat_mode (the pass that makes all state embeddings
 * ahead of the chunks does not exist there); [batch, timesteps, d_model] embeddings or flattened maps beyond 2 GiB; a slot table
 * without image slots; dev_obs_seq NULL with vector slots in the table.
 * Everything runs on the call's stream ahead of the first chunk.  Out of scope: overlapping the CNN with the chunk lanes; a
 * matrix-core convolution (the step and the contexts keep one arithmetic). */
int32_t lram_prefill_frames(lram_engine* e, const uint8_t* dev_frames, int32_t channels, int32_t height, int32_t width,
                            const float* dev_obs_seq, const float* dev_rtg_seq, const float* dev_reward_seq, int32_t timesteps,
                            const int32_t* host_lengths, int32_t append, const uint8_t* dev_reset_mask, int32_t discrete,
                            float* dev_actions, int32_t* dev_tokens, void* stream);
int32_t lram_score_frames(lram_engine* e, const uint8_t* dev_frames, int32_t channels, int32_t height, int32_t width,
                          const float* dev_obs_seq, const float* dev_rtg_seq, const float* dev_reward_seq, int32_t timesteps,
                          const int32_t* host_lengths, int32_t append, const uint8_t* dev_reset_mask, int32_t discrete,
                          const float* dev_target_actions, const int32_t* dev_target_tokens, const uint8_t* dev_valid, int32_t over,
                          double temperature, float* dev_actions, int32_t* dev_tokens, float* dev_logp, float* dev_logits,
                          void* stream);

/* Slot table: per env slot the head mode, the number of action dims in use and the observation kind -- what the reference's
 * evaluation loop hands every call for ONE env (`env_act_dim`, `is_discrete`: src/callbacks/evaluation.py:90-138; the head
 * treats the two kinds differently, multi_domain_discrete_dt_model.py:83-108), here for every slot of one batch, so that envs
 * of several domains (Atari / Procgen frames with 18 discrete actions beside Meta-World / DMControl vectors with 1-8 tokenised
 * action dims) step together.  Host arrays of `batch` entries; NULL, NULL clears the table.  flags[b]: LRAM_SLOT_* bits;
 * act_dim[b] in 1 .. cfg.act_dim, a discrete slot has act_dim 1.
 *   - Not a hot-path call: synchronises the device, drops a captured graph, keeps a host copy (it gives every env slice its
 *     range of frames) and a device copy (read by the head launches).  lram_state_alloc clears the table.  lram_config and
 *     LRAM_ABI_VERSION are unchanged.  A refused table leaves the one in effect as it was.
 *   - Errors: an unknown flag bit; act_dim out of range; a discrete slot with act_dim != 1 or with cfg.n_discrete == 0.  Image
 *     slots without `embed_image.*` weights fail at the first lram_step_slots call that needs them.
 *   - Head output for slot b (discrete = LRAM_HEAD_PER_SLOT or lram_step_slots), the same in argmax and sampling mode:
 *       continuous slot: columns j < act_dim[b] hold what discrete = 0 writes;
 *       discrete slot:   column 0 holds what discrete = 1 writes;
 *       every other column: actions = 0.0f, tokens = -1, written on every call.
 *   - Sampling: the Philox counter stays (slot_base + s, j, d), so a slot of a mixed batch draws what the same slot of a
 *     homogeneous batch draws.  Armed with top_k > n_discrete while the table holds a discrete slot: the call fails (as a
 *     discrete = 1 call does).
 *   - discrete = LRAM_HEAD_PER_SLOT is accepted by lram_step, lram_step_images and lram_prefill (head of the last timestep) and
 *     fails without a table.  In graph mode it is one more value of the captured step's key.
 *   - Together with the Mamba repeated-forward mode (lram_set_compat_mode, mamba_repeat > 1) it is refused: the reference
 *     advances the state env_act_dim times there (src/algos/decision_mamba.py:107-122), which differs per slot and is not a
 *     batchable trajectory.
 * lram_get_slot_table copies the table in effect back (any pointer may be NULL) and fails when none is set. */
int32_t lram_set_slot_table(lram_engine* e, const uint8_t* host_flags, const uint8_t* host_act_dim);
int32_t lram_get_slot_table(lram_engine* e, uint8_t* host_flags, uint8_t* host_act_dim, int32_t* n_image_slots);

/* Allowed-action sets: which vocabulary tokens an env slot may take.  The reference cuts every env's row at `discrete_actions`
 * alike (get_action_from_logits, src/algos/models/multi_domain_discrete_dt_model.py:83-88); the envs differ from that (Procgen
 * has 15 actions, an Atari game on its minimal set 4 .. 18 that are no prefix of the full set, Dark-Room 5), and under sampling
 * a slot would be handed an action its env does not have.
 *   host_bits  host uint32[batch, words], words = ceil(cfg.n_vocab / 32): bit t & 31 of word t >> 5 set = token t is allowed.
 *              NULL clears the mask.  Bits at or above n_vocab are ignored and read back as 0.
 * The rule, the same in every head kernel: a column in use (env slot b, action dim j) with the selectable range [0, n)
 * (n = n_discrete on a discrete column, n_vocab otherwise) works on the SUB-ROW x[i], i in S_b within [0, n), in vocabulary order,
 * exactly as if the reference's function had been handed that sub-row, and maps the answer back to vocabulary indices:
 *   - greedy (the argmax head, greedy slots of the sampling head, the greedy token / action of the score entries): the
 *     first index of the sub-row's maximum;
 *   - a draw (lram_set_sampling): sample_from_logits on the sub-row -- the quantile ranks its m = |S_b within [0, n)| values, top-k
 *     keeps among them (a top_k above m keeps all), weights and inverse CDF in vocabulary order.  The Philox counter is
 *     unchanged, so the uniform of a (slot, dim, draw) does not depend on the mask.  The argmax rule takes over where the
 *     sub-row holds a NaN, its maximum is +-inf, or nothing is left.  Disallowed logits are invisible, a NaN included;
 *   - lram_score_last_sampled: under that distribution; a disallowed token scores -inf, on the argmax rule the sub-row's
 *     argmax scores 0;
 *   - over = 1 (the selectable range) of lram_score* / lram_score_last: maximum, NaN flag and sum over the sub-row; a target
 *     outside it scores -inf;
 *   - over = 0 (the vocabulary): unchanged -- all n_vocab logits, the reference's cross-entropy; the greedy token and action
 *     returned beside it still obey the mask;
 *   - raw logits (the `logits` output of the score entries, lram_get_taps) are never altered.
 * A token returned for a masked slot is always allowed; a mask that allows everything equals no mask, bit for bit.
 *   - Not a hot-path call: like lram_set_slot_table it keeps a host copy and a device copy, synchronises and drops a captured
 *     graph.  lram_state_alloc drops the mask.  lram_config and LRAM_ABI_VERSION are unchanged.
 *   - The mask stays with the slot INDEX, as the slot table and the sampling table do: lram_state_copy_slots / swap_slots /
 *     load_slots do not move it.  It applies to whatever rows a call takes (the live prefix, context rows, env slices).
 *   - Refused, with nothing changed: words != ceil(n_vocab / 32); a slot that allows nothing inside its selectable range (with
 *     a slot table the slot's own flag decides the range, without one it is [0, n_vocab)).  While some slot allows nothing
 *     below n_discrete, a call with discrete = 1 is refused before anything is launched; and lram_set_slot_table is refused
 *     while a mask is in effect if the new table would leave some slot an empty sub-row.
 * lram_get_action_mask copies the mask in effect back (host_bits may be NULL; zeros when none is set) and sets *on to 0 / 1. */
int32_t lram_set_action_mask(lram_engine* e, const uint32_t* host_bits, int32_t words);
int32_t lram_get_action_mask(lram_engine* e, uint32_t* host_bits, int32_t words, int32_t* on);
/* lram_sample_rows / lram_score_tokens with one allowed set per row (test / evidence entries of the rule above):
 * dev_mask device uint32[rows, words], words = ceil(n / 32) resp. ceil(n_vocab / 32); every row's sub-row must be non-empty
 * (not checked: the sets are device data; an empty one yields token INT32_MAX). */
int32_t lram_sample_rows_masked(const float* dev_logits, int64_t rows, int32_t n, int64_t ld, const uint8_t* dev_mode,
                                const double* dev_temperature, const int32_t* dev_top_k, const double* dev_top_p,
                                const double* dev_uniform, const int32_t* dev_tokens_in, int32_t* dev_tokens_out,
                                float* dev_logp_out, const uint32_t* dev_mask, int32_t words, void* stream);
int32_t lram_score_tokens_masked(const float* dev_logits, int64_t rows, int32_t act_dim, int32_t n_vocab, int32_t n_discrete,
                                 int32_t action_channels, float tok_min, float tok_max, int32_t discrete,
                                 const float* dev_target_actions, const int32_t* dev_target_tokens, const uint8_t* dev_valid,
                                 int32_t over, double temperature, float* dev_actions, int32_t* dev_tokens, float* dev_logp,
                                 const uint32_t* dev_mask, int32_t words, void* stream);

/* One env-step of a mixed batch: per slot the observation is a vector or a frame and the head is continuous or discrete, as the
 * slot table says -- the batched form of the reference's forward, which embeds `states` through embed_state or embed_image
 * depending on the env (online_decision_transformer_model.py:463-530) and reads the head as the env's kind asks
 * (multi_domain_discrete_dt_model.py:83-108).
 *   dev_obs    device float[batch, state_dim]: rows of image slots are never used (any bit pattern); NULL when every slot is
 *              an image slot
 *   dev_images device uint8[n_image_slots, C, H, W]: frame k belongs to the k-th image slot in ascending slot order (NULL if
 *              the table holds none)
 * Other arguments as lram_step; the head mode is per slot.  Per env slice and on the slice's stream: the state Linear over the
 * slice's rows, the IMPALA CNN over the slice's frames (a contiguous range), and a scatter of the CNN rows into the image
 * slots' state tokens; a slice without image slots launches no CNN.  Runs launch-per-kernel also in graph mode (a captured
 * step would pin the frame buffer, as in lram_step_images).  Fails without a table. */
int32_t lram_step_slots(lram_engine* e, const float* dev_obs, const uint8_t* dev_images, int32_t channels, int32_t height,
                        int32_t width, const float* dev_rtg, const float* dev_reward, const uint8_t* dev_reset_mask,
                        float* dev_actions, int32_t* dev_tokens, void* stream);

/* Observation front end on the device: native obs [batch, n_native] -> model input [batch, state_dim].
 * dev_inv_index == NULL: zero-pad (DecisionXLSTM.pad_inputs, src/algos/decision_xlstm.py:16-19); otherwise
 * int32[state_dim] giving, per output dim, the native column it is filled from or -1 (DMControl full-space
 * mapping, src/envs/dmcontrol_utils.py:35-59; Mimicgen, mimicgen_utils.py:190-197).  Optional fused
 * normalisation (x - mean) / std over the padded vector (src/algos/decision_transformer_sb3.py:650-651). */
int32_t lram_pad_obs(const float* dev_native, int32_t n_native, const int32_t* dev_inv_index, const float* dev_mean,
                     const float* dev_std, float* dev_out, int32_t batch, int32_t state_dim, void* stream);

/* lram_pad_obs with one index / mean / std row per slot: tables [n_rows, state_dim] (dev_inv_index NULL: zero-pad for every
 * slot), dev_slot_row int32[batch] in 0 .. n_rows - 1 (a slot with any other value gets zeros).  One batch of envs whose
 * domains map their observations differently (a Meta-World zero-pad beside the DMControl full-space mapping,
 * src/envs/dmcontrol_utils.py:35-59).  With n_rows = 1 and dev_slot_row all zero it equals lram_pad_obs bit for bit. */
int32_t lram_pad_obs_slots(const float* dev_native, int32_t n_native, const int32_t* dev_slot_row, const int32_t* dev_inv_index,
                           const float* dev_mean, const float* dev_std, int32_t n_rows, float* dev_out, int32_t batch,
                           int32_t state_dim, void* stream);

/* Diagnostic: runs the mLSTM front-end kernel beside a bf16x3 GEMM on a second stream `iters` times and counts
 * output elements that differ from a solo run (must be 0; see lram_amd/csrc/selftest.hip for the gfx950
 * packed-fp32 / bf16-MFMA co-execution hazard this guards against). */
int32_t lram_selftest_concurrent(int32_t iters, int64_t* n_diff);
/* STREAM-like device copy (float4), used by bench.py to measure the achievable HBM rate on the box. */
int32_t lram_stream_copy(float* dev_dst, const float* dev_src, size_t numel, void* stream);

/* Measurement aid: read-only stream over `numel` floats (a multiple of 1 Mi) with the access shape of the lazy mLSTM read
 * pass (mlstm_lazy.hip: whole 1 KiB rows per wave, several rows in flight per lane, non-temporal loads) and none of its
 * arithmetic; per-workgroup sums are accumulated into dev_sink (1024 floats).  The practical ceiling for "read the state
 * once" that bench.py reports beside the read pass's rate. */
int32_t lram_stream_read(const float* dev_buf, size_t numel, float* dev_sink, void* stream);

/* Measurement aid: in-place read-modify-write stream (x *= 1) over `numel` floats (a multiple of 65536) with the
 * access pattern of the mLSTM cell kernel and none of its arithmetic -- the practical ceiling for "read the state
 * once, write it once" that bench.py reports beside the cell kernel's rate. */
int32_t lram_stream_rmw(float* dev_buf, size_t numel, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRAM_HIP_H */
