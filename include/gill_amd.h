/* libgill_amd — C ABI of the MI355X-native GILL image-generation hot path.
 *
 * The reference (kohjingyu/gill) has no FFI seam: its "operator API" is the Python class surface
 * gill.models.{load_gill, GILL, GILLModel} + gill.layers.TextFcLayer, and every FLOP runs inside
 * transformers/diffusers/torch.  This header is the boundary the Python mirror (gill_amd/) binds
 * with ctypes; each entry point names the reference call it replaces.
 *
 * Conventions
 *  - All data pointers are DEVICE pointers borrowed for the duration of the call (torch tensors'
 *    data_ptr()); the caller allocates every output.  Exceptions are marked "host".
 *  - Work is enqueued on the caller-supplied stream (a hipStream_t passed as void*; NULL = the
 *    default stream).  Nothing synchronises the device unless stated.
 *  - Every function returns 0 on success; on failure a negative code, with a thread-local message
 *    retrievable through gill_last_error().  No C++ exception crosses this boundary.
 *  - bf16 tensors are raw uint16 bit patterns.  Shapes are row-major, last index fastest.
 *  - Handles are not re-entrant (the reference serialises requests: demo/app_gradio.py:217).
 */
#ifndef GILL_AMD_H
#define GILL_AMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GILL_DTYPE_BF16 0
#define GILL_DTYPE_F32 1
#define GILL_DTYPE_F16 2

/* One named weight tensor (state-dict entry).  `data` is a device pointer; it is copied /
 * re-laid-out into handle-owned HBM during *_create and not referenced afterwards. */
typedef struct {
  const char* name;
  const void* data;
  int32_t dtype; /* GILL_DTYPE_* */
  int32_t ndim;
  int64_t shape[4];
} gill_tensor;

const char* gill_last_error(void);
int gill_version(void);

/* ------------------------------------------------------------------------------------------
 * Stage 1 — frozen OPT decoder.  Replaces self.lm(inputs_embeds=..., output_hidden_states=True)
 * of transformers OPTForCausalLM at gill/models.py:363-365 (batched) and :465 (generate loop).
 * State-dict names are those of OPTForCausalLM ("model.decoder.layers.N.self_attn.q_proj.weight").
 * ------------------------------------------------------------------------------------------ */
typedef struct gill_opt gill_opt;
typedef struct {
  int32_t vocab_size;   /* rows of embed_tokens after resize_token_embeddings (models.py:73) */
  int32_t hidden_size;  /* == word_embed_proj_dim (no project_in/out: every OPT but 350m) */
  int32_t num_layers;
  int32_t num_heads;
  int32_t ffn_dim;
  int32_t max_positions; /* 2048; learned positions carry the +2 offset */
  int32_t max_batch;     /* workspace sizing */
  int32_t max_seq;
} gill_opt_config;

int gill_opt_create(gill_opt** out, const gill_opt_config* cfg, const gill_tensor* weights, int n_weights);
void gill_opt_destroy(gill_opt* h);

/* Quantised decoder ("w8"): gill_opt_create with a weight mode.  GILL_OPT_BF16 is gill_opt_create itself.  GILL_OPT_W8 is weight-only
 * fp8: per decoder layer the four matrices [q|k|v] stacked, out_proj, fc1 and fc2 (embeddings, positions, lm_head, biases and LayerNorms
 * are untouched) are quantised from their bf16-rounded values, per output row n:
 *   e[n] = ceil(log2(max_k |w[n][k]| / 448)), s[n] = 2^e[n] (an all-zero row: s = 1; e is kept >= -100),
 *   w8[n][k] = e4m3fn(w[n][k] / s[n]), OCP e4m3, round to nearest even; max|w / s| lies in (224, 448]: nothing saturates.
 * The quantised model is the model whose weights are w8[n][k] * s[n].  Every e4m3 code times a power of two is a bf16 number, so it is an
 * exact bf16 model, and the handle keeps BOTH copies of those matrices: the dequantised bf16 values, in the layouts of a bf16 handle, and
 * the fp8 bytes + fp32 scales: about 1.5 x the decoder weights of a bf16 handle in memory (OPT-6.7b: about 19 GB instead of 12.9).
 *   gill_opt_decode_step at B <= gill_w8_max_rows() runs its four linears per layer on the fp8 bytes (csrc/linear_w8.hip: bf16
 *     activations, weights converted to bf16 in registers, fp32 accumulation; half the weight bytes per step): the ragged loop of
 *     generate_batch.
 *   gill_opt_forward_cached with past_len > 0 and B * T_new <= gill_w8_max_rows() runs the same four linears on the bytes, with
 *     self-attention as projection -> gill_attention_append (every row at length past_len) -> out-projection: the decode steps of
 *     generate(), its 8-token [IMG] block at B = 1 included.  The cache is the one layout either way: routed and un-routed calls of a
 *     sequence may alternate.
 *   gill_opt_decode_step and gill_opt_forward_cached at more rows, gill_opt_forward_cached at past_len = 0 (the prefill) and every other
 *     entry (forward, img_hidden*, prefill_ids, forward_loss, the logits) run the kernels of a bf16 handle on the dequantised matrices:
 *     the same model, no speed-up.
 * gill_opt_weight_mode: the handle's mode.  gill_opt_decode_uses_w8 / gill_opt_cached_uses_w8: host-only, 1 when gill_opt_decode_step at
 * this B / gill_opt_forward_cached at this (B, T_new, past_len) takes the fp8 path (the functions the engine itself branches on), else 0. */
enum { GILL_OPT_BF16 = 0, GILL_OPT_W8 = 1 };
int gill_opt_create_ex(gill_opt** out, const gill_opt_config* cfg, const gill_tensor* weights, int n_weights, int weight_mode);
int gill_opt_weight_mode(const gill_opt* h);
int gill_opt_decode_uses_w8(const gill_opt* h, int B);
int gill_opt_cached_uses_w8(const gill_opt* h, int B, int T_new, int past_len);
int gill_w8_max_rows(void);     /* W8_MAX_ROWS: the most activation rows of one fp8 linear (16) */

/* Operator entries of the w8 format (tests).  Bytes are in the kernel's order [N / 16][K / 64][64][16]: byte (n, k) at
 * ((n / 16) * (K / 64) + k / 64) * 1024 + ((k % 64) / 16 * 16 + n % 16) * 16 + k % 16.  N and K multiples of 64.
 *   gill_op_w8_quant:   w (N,K) bf16 row-major -> w8 (N*K bytes), scale (N) fp32.
 *   gill_op_w8_dequant: -> out (N,K) bf16, row-major (blk64 = 0) or 64 x 64-blocked [N/64][K/64][64][64] (blk64 = 1); w8 * s, exact.
 *   gill_op_linear_w8:  y = act(s[n] * sum_k A[m][k] * w8[n][k] + bias[n]) (+ resid_f32[m][n]); A (M,K) bf16, 1 <= M <= gill_w8_max_rows();
 *     act 0 = none, 1 = ReLU; out (M,N) bf16 or fp32 (out_f32); resid fp32, may be out itself.  splitk: 0 = the launcher's own rule (a function
 *     of N and K alone), 1 = unsplit, k > 1 = k slices of K.  With ln_out_bf16 (then out is fp32, resid == out, act 0, bias set): fp32 partials +
 *     the engine's reducer: out = resid + sum + bias, ln_out = LayerNorm(out; ln_g, ln_b, eps 1e-5) in bf16.  Row m's result does not depend on M
 *     or on the other rows.  Bad arguments are reported before anything is launched. */
int gill_op_w8_quant(const void* w_bf16, int N, int K, void* w8, float* scale, void* stream);
int gill_op_w8_dequant(const void* w8, const float* scale, int N, int K, int blk64, void* out_bf16, void* stream);
int gill_op_linear_w8(const void* A_bf16, const void* w8, const float* scale, const float* bias, const float* resid_f32, void* out, int M, int N,
                      int K, int act, int out_f32, int splitk, const float* ln_g, const float* ln_b, void* ln_out_bf16, void* stream);

/* input_embeddings(ids): models.py:180 / :620.  ids (B*T) int64 -> out (B*T, D) bf16. */
int gill_opt_embed(gill_opt* h, const int64_t* ids, int n, void* out_bf16, void* stream);

/* Full causal forward over right-padded sequences, no attention mask (models.py:363-365).
 *   inputs_embeds (B,T,D) bf16  ->  hidden_out (B,T,D) fp32 = hidden_states[-1] (post final LN).
 * hidden_out may be NULL when only gathered rows are wanted (see gill_opt_img_hidden). */
int gill_opt_forward(gill_opt* h, const void* inputs_embeds_bf16, int B, int T, float* hidden_out, void* stream);

/* KV-cached continuation of the same forward for the decode loop of GILLModel.generate (models.py:464-530; the reference
 * re-runs the whole sequence every step with use_cache unset).  inputs_embeds (B,T_new,D) bf16 are the tokens
 * past_len .. past_len+T_new-1 of each sequence; their keys/values are appended to the handle's cache and they attend to
 * cache[0, past_len) plus, causally, to each other.  past_len = 0 starts a new sequence (prefill).  The caller keeps B
 * fixed and past_len equal to the number of tokens already fed.  hidden_out (B,T_new,D) fp32 = hidden_states[-1] rows. */
int gill_opt_forward_cached(gill_opt* h, const void* inputs_embeds_bf16, int B, int T_new, int past_len, float* hidden_out,
                            void* stream);

/* The fast path of GILLModel.forward(mode='generation') (models.py:180-183, 384-385):
 *   ids (B,T) int64 right-padded, last_idx (B) int32 HOST array = caption_len-1;
 *   raw_out (B,8,D) bf16 = hidden_states[-1][i, last-7:last+1];  emb_out (B,8,D) bf16 = input_embs slice. */
int gill_opt_img_hidden(gill_opt* h, const int64_t* ids, const int32_t* last_idx_host, int B, int T, int num_tokens,
                        void* raw_out_bf16, void* emb_out_bf16, void* stream);

/* gill_opt_img_hidden for interleaved image + text prompts (gill/models.py:606-613, 625: the visual embeddings of an image take
 * the place of token embeddings in inputs_embeds).  extra_rows (n_extra, D) bf16 holds those rows; an id < 0 selects row
 * -(id + 1) of it instead of an embed_tokens row, both for the emb_out gather and for the position-added fp32 stream.  The ids
 * live on the device, so the range is the caller's to check: an id below -n_extra reads row n_extra - 1 (clamped, like ids past
 * the vocabulary).  n_extra == 0 (extra_rows may be NULL) is gill_opt_img_hidden itself, bit for bit. */
int gill_opt_img_hidden_ex(gill_opt* h, const int64_t* ids, const int32_t* last_idx_host, int B, int T, int num_tokens,
                           const void* extra_rows_bf16, int n_extra, void* raw_out_bf16, void* emb_out_bf16, void* stream);

/* logits[:, -1, :] of the tied lm_head for the generate loop (models.py:470):
 *   hidden (B,T,D) fp32 from gill_opt_forward -> logits_out (B, vocab) fp32.  Any B >= 1: the rows go through the GEMV
 *   8 at a time, each row's arithmetic independent of the others (a row's logits do not depend on B). */
int gill_opt_last_logits(gill_opt* h, const float* hidden, int B, int T, float* logits_out, void* stream);

/* The decision half of the generate loop, on the device (models.py:471-520).
 * gill_decode_rule holds the arguments of the [IMG] logit rule (:476-489) as GILLModel.generate has them:
 *   ret_ids / gen_ids = retrieval_token_idx / gen_token_idx (at most 16 each; negative ids index from the end, as in torch),
 *   step = the loop index i, min_word_tokens, ret_scale / gen_scale / filter_value = the Python floats,
 *   ret_eq_gen = (retrieval_token_idx == gen_token_idx), the assert at :519. */
typedef struct gill_decode_rule {
  int32_t n_ret;
  int32_t ret_ids[16];
  int32_t n_gen;
  int32_t gen_ids[16];
  int32_t step;
  int32_t min_word_tokens;
  int32_t ret_eq_gen;
  double ret_scale;
  double gen_scale;
  double filter_value;
} gill_decode_rule;

/* Greedy step (:470-491, :498, :518-529): lm_head as gill_opt_last_logits -> logits_out (B, vocab) fp32, the rule applied in
 * place (what output_logits holds, :472-477), torch.argmax per row; at B == 1 a pick equal to ret_ids[0] emits all n_ret ids
 * (:518-520).  The emitted ids go to tokens (B, ld) int64 at columns col.., their count (1, or n_ret; -1 when [IMG0] was picked
 * with ret_eq_gen == 0: the reference's AssertionError) to *n_out (device int32), and their input_embeddings rows (bf16, as
 * gill_opt_embed) to next_embeds: row b at B > 1 ((B,1,D)), rows 0..n-1 at B == 1 ((1,max(1,n_ret),D)).  No host wait. */
int gill_opt_next_token(gill_opt* h, const float* hidden, int B, int T, const gill_decode_rule* rule, float* logits_out,
                        int64_t* tokens, int ld, int col, int32_t* n_out, void* next_embeds_bf16, void* stream);

/* The same decision on caller-supplied logits (B, vocab) fp32, modified in place (:476-498, :518-520). */
int gill_opt_pick_token(gill_opt* h, float* logits, int B, const gill_decode_rule* rule, int64_t* tokens, int ld, int col,
                        int32_t* n_out, void* next_embeds_bf16, void* stream);

/* Sampled step, first half (:470-489): lm_head + the rule in place -> logits_out (B, vocab) fp32. */
int gill_opt_decode_logits(gill_opt* h, const float* hidden, int B, int T, const gill_decode_rule* rule, float* logits_out,
                           void* stream);

/* Sampled step, second half (:500-512): out = in / temperature, then filter_value on every token the sort / softmax / cumsum
 * top-p rule removes (only when top_p < 1; vocab <= 65536).  reciprocal = 0: correctly rounded fp32 division (torch on the
 * CPU); reciprocal = 1: in * fp32(1 / temperature) (torch on the GPU for a tensor divided by a Python float).  Out of place,
 * deterministic: the same input gives the same bits on every call. */
int gill_opt_filter_logits(gill_opt* h, const float* in, float* out, int B, double temperature, double top_p,
                           double filter_value, int reciprocal, void* stream);

/* The seeded draw: temperature / top-p sampling decided on the device, in the place of torch.multinomial (:514).  For row b of a
 * call, with x the post-rule logits, T = temperature > 0 and 0 < top_p <= 1:
 *   y_c = x_c / T (correctly rounded fp32: the reciprocal = 0 arm of gill_opt_filter_logits); mx = max_c y_c;
 *   e_c = exp(y_c - mx), 0 where y_c = -inf: the values gill_opt_filter_logits forms, to the bit.  With top_p < 1 the kept set is
 *   that entry's (one device function serves both); with top_p == 1 every token is kept.
 *   u_c = (2 * (w >> 9) + 1) * 2^-24 with w the output word c & 3 of Philox4x32-10 (multipliers D2511F53 / CD9E8D57, key
 *   increments 9E3779B9 / BB67AE85) at key (seed & 0xffffffff, seed >> 32) and counter (c >> 2, row0 + b, draw, 0): exact in
 *   fp32 and strictly inside (0, 1).
 *   key_c = e_c / -logf(u_c) (accurate logf, correctly rounded division); the token is the argmax of key_c over the kept columns,
 *   larger key first, then lower index: the exponential race, P(token = c) = e_c / sum of the kept e.
 * A row's token is a function of (seed, row0 + b, draw, that row's logits) alone: repeatable bit for bit, independent of the batch
 * it runs in, and safe at any temperature.  A row with no finite maximum (it holds a NaN or +inf, or is all -inf) draws nothing: its
 * token is torch.argmax's pick on y (first NaN, else larger value, else lower index).  What follows the pick is gill_opt_next_token's
 * to the byte: the [IMG] forcing at B == 1, -1 in *n_out when ret_eq_gen == 0, tokens, *n_out and the bf16 embedding rows.
 * temperature <= 0, top_p outside (0, 1], vocab > 65536, draw or row0 < 0, a null pointer or a token buffer that is too short are
 * errors, reported before anything is enqueued. */
typedef struct gill_decode_sampler {
  uint64_t seed;
  int32_t draw;    /* the loop step */
  int32_t row0;    /* id of row 0 */
  double temperature;
  double top_p;
} gill_decode_sampler;

/* Twin of gill_opt_next_token: lm_head -> logits_out, the rule in place (logits_out keeps the post-rule, pre-temperature values,
 * what output_logits holds), then the draw.  No host wait. */
int gill_opt_sample_token(gill_opt* h, const float* hidden, int B, int T, const gill_decode_rule* rule,
                          const gill_decode_sampler* sampler, float* logits_out, int64_t* tokens, int ld, int col, int32_t* n_out,
                          void* next_embeds_bf16, void* stream);

/* Twin of gill_opt_pick_token: the caller's logits (B, vocab) fp32, modified by the rule only. */
int gill_opt_draw_token(gill_opt* h, float* logits, int B, const gill_decode_rule* rule, const gill_decode_sampler* sampler,
                        int64_t* tokens, int ld, int col, int32_t* n_out, void* next_embeds_bf16, void* stream);

/* Host only, no GPU: u_c of the draw above for c in [first, first + count), first + count <= 65536, from the code the kernel runs. */
int gill_decode_uniforms(uint64_t seed, int32_t row, int32_t draw, int32_t first, int32_t count, float* u_out);

/* ---- Ragged batched decoding: every row of the batch at its own length (one dialogue per row). ----
 *
 * Decode attention with append, the operator under gill_opt_decode_step.  One new token per row: q, k_new, v_new are rows of ld bf16
 * elements with head h at column h * d (d = 64, 80 or 128); K (B,H,pitch,d) and Vt (B,H,round_up(d,32),pitch) are the cache in the
 * layout of gill_opt_forward_cached; lens (B) int32 on the DEVICE.  With n = lens[b]: the new key / value are stored at slot n and
 * o (B, H*d) bf16 = softmax(q . [K[0..n-1]; k_new] / sqrt(d)) . [V[0..n-1]; v_new].  Slots beyond n are excluded by selection whatever
 * they hold.  n outside [0, pitch - 1] is clamped into it and flags[b] (device int32, nullable) is set to 1; nothing outside the
 * buffers is touched.  A row's output is a fixed function of its own operands and length: the same bits at any B, on any run. */
int gill_attention_decode(const void* q, const void* k_new, const void* v_new, int ld, void* K, void* Vt, const int32_t* lens,
                          void* o, int B, int H, int d, int pitch, int32_t* flags, void* stream);

/* Decode attention with a multi-token append, the operator under gill_opt_forward_cached on a w8 handle (below).  Row b brings nq
 * consecutive new tokens, 1 <= nq <= gill_w8_max_rows(), at its own cache length n = lens[b]: q, k_new, v_new and o hold B * nq rows (ld
 * elements; o: H*d), row b * nq + i the token n + i of sequence b; K, Vt, lens, d and flags as in gill_attention_decode.  Token i's key /
 * value are stored at slot n + i (and the ones-row entry Vt[b][h][d][n + i] = 1 where round_up(d,32) > d), and
 *   o[b * nq + i] = softmax(q_i . [K[0..n-1]; k_0..k_i] / sqrt(d)) . [V[0..n-1]; v_0..v_i].
 * Slots at or beyond n + nq, and for token i the slots n + i + 1 .., are excluded by selection whatever they hold.  n outside
 * [0, pitch - nq] is clamped into it and flags[b] is set to 1; nothing outside the buffers is touched.  A row's output and cache are, bit
 * for bit, those of nq successive gill_attention_decode calls, the i-th with lens = n + i: the same bits at any B, under any grouping of
 * the tokens into calls, on any run; nq == 1 is gill_attention_decode itself.  nq outside its range, a misaligned pointer or an
 * unsupported d are errors, reported before anything is launched. */
int gill_attention_append(const void* q, const void* k_new, const void* v_new, int ld, void* K, void* Vt, const int32_t* lens,
                          void* o, int B, int nq, int H, int d, int pitch, int32_t* flags, void* stream);

/* One decode step of B rows at B different lengths.  new_embeds (B,1,D) bf16: row b's token sits at position lens_dev[b] (device
 * int32): it takes position embedding 2 + lens_dev[b], its key / value go to slot lens_dev[b] of row b's cache and it attends to
 * slots 0 .. lens_dev[b].  len_bound is the host's upper bound on max(lens) + 1, checked against max_seq and the position table
 * before anything is enqueued.  The layers are those of gill_opt_forward_cached with self-attention as projection ->
 * gill_attention_decode -> out-projection.  hidden_out (B,1,D) fp32 = hidden_states[-1].  The step neither writes nor advances
 * lens_dev (the ragged decision below owns it).  A length the device holds beyond the cache is clamped and reported through the
 * rows' flags by the next ragged decision.  No host wait. */
int gill_opt_decode_step(gill_opt* h, const void* new_embeds_bf16, const int32_t* lens_dev, int B, int len_bound, float* hidden_out,
                         void* stream);

/* Prefill for the ragged loop: ids (B,Tmax) int64 on the device, right-padded (an id < 0 selects row -(id + 1) of extra_rows
 * (n_extra, D) bf16, as in gill_opt_img_hidden_ex), embedded and run through gill_opt_forward_cached's pass at past_len = 0.
 * hidden_out (B,Tmax,D) fp32; row b's last real row is len[b] - 1.  Pad positions write keys / values at slots >= len[b]: the first
 * decode step overwrites slot len[b] and nothing beyond a row's length is ever selected. */
int gill_opt_prefill_ids(gill_opt* h, const int64_t* ids, int B, int Tmax, const void* extra_rows_bf16, int n_extra, float* hidden_out,
                         void* stream);

/* Ragged decode state: int32 words on the device, field-major, [6][B] followed by one word:
 *   state[0*B + b] len     position of row b's newest token: the one whose hidden row the next decision reads.  An emitting
 *                          decision advances it to the emitted token's position, which is where gill_opt_decode_step (lens_dev =
 *                          state) then stores that token: the row's cache length at that step.  Start: prompt length - 1.
 *   state[1*B + b] step    decisions taken (the loop index i of the one-sequence generate())
 *   state[2*B + b] forced  index into ret_ids of the next forced id, 0 = no [IMG] block pending
 *   state[3*B + b] n_tok   ids emitted into tokens[b][..]
 *   state[4*B + b] row_id  the row's Philox key (gill_decode_sampler.row0 of the one-sequence draw)
 *   state[5*B + b] flags   1: [IMG0] picked with ret_eq_gen == 0 (the reference's AssertionError); 2: a length was clamped to the
 *                          cache; 4: the token buffer was full
 *   state[6*B]             rows still active (start: B, or the number of rows with max_steps > 0)
 * One launch per iteration, every row one of three ways:
 *   forced > 0:  emits ret_ids[forced], forced + 1 (0 after the last id); no decision: step stands, the logits are not touched;
 *   else step >= max_steps: finished, nothing changes;
 *   else: the rule with rule->step replaced by the row's step, torch.argmax (sampler == NULL) or the seeded draw of
 *         gill_opt_sample_token keyed (seed, row_id, draw = step) (sampler->draw and ->row0 are not read); a pick of ret_ids[0]
 *         with n_ret > 1 sets forced = 1 (ret_eq_gen == 0: flag 1 instead); step + 1.
 * An emitting row stores its id at tokens[b][n_tok++] (tokens (B, ld) int64), the id's input_embeddings row at next_embeds[b]
 * ((B,1,D) bf16) and advances len.  The active count drops by one when a row emits its last id.  A row's ids are a function of its
 * own logits and state: they are those of the one-sequence loop, an [IMG] block taking n_ret iterations.  No host wait.
 * hidden (B,1,D) fp32: the rows the decision reads (the prefill's rows len[b] - 1 gathered by the caller, then gill_opt_decode_step's
 * output); lm_head as gill_opt_last_logits (a row's logits do not depend on B) -> logits_out (B, vocab) fp32, the rule in place on
 * the rows that decide.  max_steps: decisions per row.  Argument errors are reported before anything is enqueued. */
int gill_opt_next_token_ragged(gill_opt* h, const float* hidden, int B, const gill_decode_rule* rule, int max_steps,
                               const gill_decode_sampler* sampler, float* logits_out, int32_t* state, int64_t* tokens, int ld,
                               void* next_embeds_bf16, void* stream);

/* The same decision on caller-supplied logits (B, vocab) fp32, modified by the rule only (rows that take no decision: untouched). */
int gill_opt_pick_token_ragged(gill_opt* h, float* logits, int B, const gill_decode_rule* rule, int max_steps,
                               const gill_decode_sampler* sampler, int32_t* state, int64_t* tokens, int ld, void* next_embeds_bf16,
                               void* stream);

/* ---- Dialogue sessions: a row's cache is kept across turns and extended by a turn's worth of new tokens. ----
 *
 * Ragged multi-token attention with append, the operator under gill_opt_extend.  Row b brings cu_new[b + 1] - cu_new[b] consecutive new
 * tokens at its own cache length n = lens[b]: cu_new (B + 1) int32 on the DEVICE holds the prefix sums of the per-row counts, and q, k_new,
 * v_new (rows of ld bf16 elements, head h at column h * d, d = 64, 80 or 128: the three thirds of one [total_new][3D] projection) and
 * o (H*d per row) hold total_new packed rows, row cu_new[b] + i the token n + i of sequence b.  K, Vt, lens and flags as in
 * gill_attention_decode.  Token i's key goes to slot n + i of K, its value to column n + i of Vt (and the ones-row entry
 * Vt[b][h][d][n + i] = 1 where round_up(d,32) > d, as gill_attention_append writes it: the decode kernels read the cache afterwards), and
 *   o[cu_new[b] + i] = softmax(q_i . [K[0..n-1]; k_0..k_i] / sqrt(d)) . [V[0..n-1]; v_0..v_i]      (the scale applied in fp32).
 * Slots at or beyond n + i + 1 are excluded by selection whatever they hold.  A row with no new tokens is legal and is left untouched.
 * max_new and total_new are HOST bounds on the per-row count and on cu_new[B]; they size the grid, 1 <= max_new <= pitch.  n outside
 * [0, pitch - count] is clamped into it and flags[b] is set to 1; a row whose device count exceeds max_new, or whose packed range leaves
 * [0, total_new), is treated as empty and flagged; nothing outside the buffers is touched.  Q.K^T and P.V run on bf16 MFMA with fp32
 * accumulation and an online softmax in fp32 over tiles of 32 keys (csrc/attention_extend.hip): a row's output and cache bits are a fixed
 * function of its own operands, n and count (the same at any B, at any place in the pack, on any run); they meet the accuracy bar of
 * gill_attention_append, not its bits (another reduction order).  An unsupported d, a misaligned pointer or max_new < 1 are errors,
 * reported before anything is launched. */
int gill_attention_extend(const void* q, const void* k_new, const void* v_new, int ld, void* K, void* Vt, const int32_t* lens,
                          const int32_t* cu_new, void* o, int B, int total_new, int max_new, int H, int d, int pitch, int32_t* flags,
                          void* stream);

/* The layers over packed new tokens at per-row cache lengths: a dialogue turn appended to each row's cache (the first feed of a row,
 * lens_dev[b] = 0, is its prefill, without pad rows).  Input: ids (total_new) int64 on the device (an id < 0 selects row -(id + 1) of
 * extra_rows (n_extra, D) bf16, as in gill_opt_prefill_ids), or, with ids NULL, embeds (total_new, D) bf16.  cu_new (B + 1) and lens_dev (B)
 * int32 on the device as in gill_attention_extend: packed row cu_new[b] + i is the token at position lens_dev[b] + i of row b, takes
 * position embedding 2 + lens_dev[b] + i, stores its key / value at that slot and attends to the slots up to it.  The layers are the one
 * loop of every other entry with self-attention as projection -> gill_attention_extend -> out-projection.
 *   hidden_last (B,1,D) fp32 = hidden_states[-1] of each row's last new token; rows without new tokens keep what they held.
 *   hidden_all (total_new, D) fp32, nullable: hidden_states[-1] of every new token.
 * max_new / total_new: host bounds as in gill_attention_extend (total_new <= max_batch * max_seq); len_bound: the host's upper bound on
 * max_b(lens_dev[b] + count[b]), checked against max_seq and the position table before anything is enqueued.  A length the device holds
 * beyond that is clamped and reported through the rows' flags by the next ragged decision.  The entry does not advance lens_dev.  No host
 * wait.  On a GILL_OPT_W8 handle the pass runs the dequantised bf16 matrices (the same model, the rule of the prefill: a turn has more rows
 * than the fp8 linear takes); the decode steps that follow keep their fp8 path, on the same cache. */
int gill_opt_extend(gill_opt* h, const int64_t* ids, const void* embeds_bf16, const void* extra_rows_bf16, int n_extra, const int32_t* cu_new,
                    const int32_t* lens_dev, int B, int total_new, int max_new, int len_bound, float* hidden_last, float* hidden_all,
                    void* stream);

/* ---- Candidate ranking: packed continuations scored against the rows' cached prefixes; the cache is read, never written. ----
 *
 * Fork attention, the operator under gill_opt_score_candidates.  C candidates are packed as in gill_attention_extend: cu_new (C + 1) int32 on
 * the DEVICE holds the prefix sums of their token counts, q / k_new / v_new / o hold total_new packed rows.  Candidate c names a cache row
 * p = parent[c] in [0, Bc) and sees that row's slots 0 .. n - 1, n = plen[c] (parent, plen: (C) int32 on the device).  K (Bc,H,pitch,d) and
 * Vt (Bc,H,round_up(d,32),pitch) are a bf16 cache as gill_attention_extend / gill_attention_decode leave it; they are const here.
 *   o[cu_new[c] + i] = softmax(q_i . [K[p][0..n-1]; k_0..k_i] / sqrt(d)) . [V[p][0..n-1]; v_0..v_i]      (the scale applied in fp32).
 * Slots of row p at or beyond n are excluded by selection whatever they hold (their scores are selected to -inf, and in the tile that
 * straddles n their V^T elements are replaced by zero).  n = 0 is legal (the candidate attends to itself only), a count of 0 is legal
 * (nothing is stored), candidates may come in any order, any number may share a parent and a cache row may have none.  n outside
 * [0, pitch] is clamped and flags[c] (nullable) set to 1; a parent outside [0, Bc), a count outside [0, max_new] or a packed range outside
 * [0, total_new) make the candidate empty and flagged, with no read through it; nothing outside the buffers is touched.  A candidate's
 * output bits are a fixed function of its own packed operands, K[p][0..n-1] / V[p][0..n-1] and n: the same at any C, anywhere in the
 * pack, beside any siblings, at any row index p.  The accuracy class of gill_attention_extend, not its bits: the candidate's own tokens
 * are tiled from its token 0, not from slot 0.  One candidate per 32-query wave tile (csrc/attention_fork.hip); the candidate's keys and
 * values are read from the packed rows, so gill_attention_fork_ws_bytes (host only) returns 0 today and ws may then be null.  An
 * unsupported d, a misaligned pointer, max_new < 1 or ws_bytes below the query's answer are errors, reported before anything is launched.
 * Honours GILL_OP_REPEAT. */
int64_t gill_attention_fork_ws_bytes(int C, int H, int d, int max_new);
int gill_attention_fork(const void* q, const void* k_new, const void* v_new, int ld, const void* K, const void* Vt, const int32_t* parent,
                        const int32_t* plen, const int32_t* cu_new, void* o, int C, int Bc, int total_new, int max_new, int H, int d, int pitch,
                        int32_t* flags, void* ws, int64_t ws_bytes, void* stream);

/* Branch decode attention: S sampled continuations ("branches") of cached dialogues decode ONE new token each.  q / k_new / v_new hold S rows
 * of ld bf16 elements (head h at column h * d), o is (S, H*d) bf16.  The main cache K (Bc,H,pitch,d) / Vt (Bc,H,round_up(d,32),pitch) is
 * const here; the branch cache Kb (Sb,H,bpitch,d) / Vtb (Sb,H,round_up(d,32),bpitch), bpitch % 32 == 0, Sb >= S, is written: branch s owns
 * row s.  Branches are packed in G groups of at most 32 siblings by three int32 arrays on the DEVICE: gstart (G + 1), group g holds the
 * branches gstart[g] .. gstart[g + 1] - 1; gparent (G), the main-cache row p all of them attend to; gplen (G), that row's visible length n,
 * 0 <= n <= pitch (the host splits a dialogue with more than 32 branches into several groups).  lens (S) int32 on the device is the branch's
 * total position: its own count is m = lens[s] - gplen[g], in [0, bpitch - 1].
 *   o[s] = softmax(q_s . [K[p][0..n-1]; Kb[s][0..m-1]; k_new_s] / sqrt(d)) . [V[p][0..n-1]; Vb[s][0..m-1]; v_new_s]   (the scale in fp32),
 * and k_new_s is stored at slot m of Kb[s], v_new_s at column m of Vtb[s] (no other word of the branch cache is written); the new key and
 * value come from the input rows, never from the slot they are stored to.  The prefix of a group is read once per (group, head), not once
 * per branch: the siblings are the query lanes of one MFMA tile (csrc/attention_branch.hip).  A branch's output bits and the bits it stores
 * depend only on its own q / k / v, K[p][0..n-1] / V[p][0..n-1], n, its own branch row up to m, and m: not on S, G, the group's size, its
 * siblings, its place in the pack or the index p.  Slots of row p at or beyond n and of the branch row at or beyond m are excluded by
 * selection whatever bits they hold.  n outside [0, pitch] or m outside [0, bpitch - 1] is clamped and flags[s] (nullable, S int32) set to 1
 * (a clamped n flags every branch of its group); a parent outside [0, Bc) empties the group and flags its branches; a group size outside
 * [0, 32] or a range outside [0, S] empties the group with no read through it and flags branch min(max(gstart[g], 0), S - 1); nothing outside
 * the buffers is touched.  An unsupported d (supported: 64, 80, 128), a misaligned pointer, bpitch % 32 != 0 (or above 1024) and S < 1 are
 * errors, reported before anything is launched.  Honours GILL_OP_REPEAT. */
int gill_attention_branch(const void* q, const void* k_new, const void* v_new, int ld, const void* K, const void* Vt, void* Kb, void* Vtb,
                          const int32_t* gstart, const int32_t* gparent, const int32_t* gplen, const int32_t* lens, void* o, int S, int G,
                          int Sb, int Bc, int H, int d, int pitch, int bpitch, int32_t* flags, void* stream);

/* Adopt a branch into its dialogue: copies Kb[s][h][0..count-1] to K[r][h][plen..plen+count-1] and the matching columns of Vtb[s] to Vt[r],
 * and writes the ones-row entry Vt[r][h][d][slot] = 1 where round_up(d,32) > d, as gill_attention_append does.  s, r, plen and count are
 * host values.  plen + count > pitch - 1, count > bpitch, s outside [0, Sb) and r outside [0, Bc) are errors that launch nothing;
 * count = 0 is legal. */
int gill_kv_branch_adopt(const void* Kb, const void* Vtb, void* K, void* Vt, int Sb, int Bc, int H, int d, int pitch, int bpitch, int s, int r,
                         int plen, int count, void* stream);

/* The layers over C packed candidates in fork mode, then the fused LM-head loss of every packed row.  Input as in gill_opt_extend: ids
 * (total_new) int64 on the device (an id < 0 selects row -(id + 1) of extra_rows), or, with ids NULL, embeds (total_new, D) bf16.  Packed
 * row cu_new[c] + i takes position embedding 2 + plen[c] + i and attends to the slots 0 .. plen[c] - 1 of cache row parent[c] and to the
 * rows cu_new[c] .. cu_new[c] + i (gill_attention_fork).  target (total_new) int64 on the device: the vocabulary id row r is scored
 * against, -100 to ignore it.  Outputs, all on the device, no host wait:
 *   token_logprob (total_new) fp32   logit[target] - logsumexp of the row, 0 where ignored and for rows no candidate owns
 *   token_rank (total_new) int32     nullable; the target's rank as in gill_opt_forward_loss, -1 where ignored
 *   score_sum (C) fp32, n_scored (C) int32, score_mean (C) fp32: per candidate, over its scored rows in packed order by one small kernel
 *                                    with a fixed summation order; the mean is NaN when nothing is scored (HF's mean over zero targets)
 *   hidden_all (total_new, D) fp32   nullable; hidden_states[-1] of every packed row
 *   flags (C) int32                  nullable, zeroed by the caller; 1 where gill_attention_fork clamped or emptied a candidate
 * The entry writes neither the cache nor any length and does not allocate the cache: a handle whose cache does not exist yet is an error,
 * and so is a GILL_KV_E4M3 handle (the message names the format).  On a GILL_OPT_W8 handle the pass runs the dequantised bf16 matrices,
 * the rule of gill_opt_extend.  Checked before anything is enqueued: C >= 1, total_new <= max_batch * max_seq, max_new >= 1, and len_bound,
 * the host's bound on max_c(plen[c] + count[c]), against the position table.  The same call twice gives equal bits; bit equality across
 * pack sizes is the operator's property, not this entry's (the GEMMs' split depends on the number of rows). */
int gill_opt_score_candidates(gill_opt* h, const int64_t* ids, const void* embeds_bf16, const void* extra_rows_bf16, int n_extra,
                              const int32_t* cu_new, const int32_t* parent, const int32_t* plen, const int64_t* target, int C, int total_new,
                              int max_new, int len_bound, float* token_logprob, int32_t* token_rank, float* score_sum, int32_t* n_scored,
                              float* score_mean, float* hidden_all, int32_t* flags, void* stream);

/* ---- branch decode: draw several replies per dialogue from one cached history (gill_attention_branch under the layers). ----
 *
 * gill_opt_branch_reserve allocates, on a bf16-cache handle, the per-layer branch cache for max_branches branches of up to branch_capacity
 * own tokens (bpitch = round_up(branch_capacity, 32), at most 1024) and the branches' clamp flags.  A GILL_KV_E4M3 handle is an error that
 * names the format.  max_branches is checked against every buffer a step over that many rows writes (the workspace rows max_batch * max_seq,
 * and the projection's 3 * S * D elements).  A later larger request frees and reallocates (it waits for the device); a request that fits
 * keeps the buffers.  Branch contents do not outlive the next reserve.  gill_opt_branch_bytes reports the size (0 before a reserve). */
int gill_opt_branch_reserve(gill_opt* h, int max_branches, int branch_capacity);
int64_t gill_opt_branch_bytes(const gill_opt* h);
/* gill_opt_decode_step over S branches: new_embeds (S, 1, D) bf16, row s takes position embedding 2 + lens_dev[s]; self-attention is the
 * projection, gill_attention_branch (groups gstart (G + 1), gparent (G), gplen (G) on the device; branch s owns row s of the branch cache)
 * and the out-projection; hidden_out (S, D) fp32 is hidden_states[-1] of the new rows.  The w8 linears by the rule of
 * gill_opt_decode_uses_w8(h, S).  No host wait.  Writes only the branch cache (and the branches' clamp flags); it does not allocate the main
 * cache: a handle without one is an error, as is S beyond the reserve.  len_bound: the host's bound on max_s(lens[s]) + 1, against the
 * position table. */
int gill_opt_decode_step_branch(gill_opt* h, const void* new_embeds_bf16, const int32_t* lens_dev, const int32_t* gstart, const int32_t* gparent,
                                const int32_t* gplen, int S, int G, int len_bound, float* hidden_out, void* stream);
/* gill_opt_next_token_ragged over S branches: the same decision and state (branch s draws with key (seed, row_id[s], its decision count)),
 * folding the branches' clamp flags (sized by the reserve, where gill_opt_next_token_ragged folds the max_batch words of the decode step). */
int gill_opt_next_token_branch(gill_opt* h, const float* hidden, int S, const gill_decode_rule* rule, int max_steps,
                               const gill_decode_sampler* sampler, float* logits_out, int32_t* state, int64_t* tokens, int ld,
                               void* next_embeds_bf16, void* stream);
/* gill_kv_branch_adopt over all layers: the first `count` own tokens of branch s become the slots plen .. plen + count - 1 of cache row r. */
int gill_opt_branch_adopt(gill_opt* h, int s, int r, int plen, int count, void* stream);

/* ---- e4m3 KV cache ("kv8"): the cache of the ragged decode step and of the extend pass at half its bytes. ----
 *
 * The format.  Every key row and every value row of one token and one head (d elements, d = 64, 80 or 128) is d OCP e4m3 bytes and one
 * power-of-two scale 2^e, e an int8 per (row, head, slot), by the rule of the w8 weights above applied to the row's bf16 values:
 *   e = ceil(log2(max |x| / 448)) from the maximum's mantissa and exponent, kept >= -100 (an all-zero row: e = 0), code = e4m3fn(x / 2^e),
 *   round to nearest even; max |x / 2^e| lies in (224, 448]: nothing saturates, and every code times 2^e is a bf16 number.
 * Layouts mirror the bf16 cache: K8 (B,H,pitch,d) bytes, Vt8 (B,H,round_up(d,32),pitch) bytes (rows d .. are never read as data and never
 * written: there is no ones-row), Kexp and Vexp (B,H,pitch) int8: d + round_up(d,32) + 2 bytes per (row, head, slot) instead of
 * 2 (d + round_up(d,32)).  Semantics: every key and value is rounded to its e4m3 row, THE TOKEN'S OWN INCLUDED, before any query uses it.  The
 * quantised-cache model is therefore an exact function of the token sequence, whichever way the tokens were fed (extend, single steps, alone
 * or in a batch); its tokens can differ from those of the bf16 cache.
 *
 * gill_attention_decode_kv8 / gill_attention_extend_kv8: gill_attention_decode / gill_attention_extend on that cache; q, k_new, v_new, o,
 * lens, cu_new, the bounds, the clamps and flags as there (k_new / v_new arrive as bf16 and are quantised by the kernel; the stored slots hold
 * the rule's codes and exponents).  Slots beyond a token's own are excluded by selection whatever bytes (the two NaN codes included) and
 * exponents they hold; no read leaves a (b, h) slab; nothing outside the buffers is touched.  Each is a fixed function of a row's own operands,
 * length and count: the same output and cache bits at any B, anywhere in a pack, on any run.  K8 / Vt8 16-byte aligned, Kexp / Vexp 4-byte
 * aligned.  Bad arguments are reported before anything is launched.  Both honour GILL_OP_REPEAT.
 *
 * gill_opt_set_kv_format: GILL_KV_BF16 (the default) or GILL_KV_E4M3 for the handle's cache; an error once the cache is allocated (the
 * first cached entry allocates it) and for any other value.  gill_opt_kv_format: the format.  gill_opt_kv_bytes: the bytes the cache holds
 * (all layers; K and V^T, and on an e4m3 handle the exponents), 0 before it exists.  On a GILL_KV_E4M3 handle gill_opt_decode_step and
 * gill_opt_extend run on the e4m3 cache with either weight mode; gill_opt_forward_cached and gill_opt_prefill_ids are errors that name the
 * format (their flash kernel writes and reads a bf16 cache: prefill through gill_opt_extend at lengths 0); entries without a cache are
 * untouched. */
enum { GILL_KV_BF16 = 0, GILL_KV_E4M3 = 1 };
int gill_opt_set_kv_format(gill_opt* h, int fmt);
int gill_opt_kv_format(const gill_opt* h);
int64_t gill_opt_kv_bytes(const gill_opt* h);
int gill_attention_decode_kv8(const void* q, const void* k_new, const void* v_new, int ld, void* K8, void* Vt8, void* Kexp, void* Vexp,
                              const int32_t* lens, void* o, int B, int H, int d, int pitch, int32_t* flags, void* stream);
int gill_attention_extend_kv8(const void* q, const void* k_new, const void* v_new, int ld, void* K8, void* Vt8, void* Kexp, void* Vexp,
                              const int32_t* lens, const int32_t* cu_new, void* o, int B, int total_new, int max_new, int H, int d, int pitch,
                              int32_t* flags, void* stream);

/* ------------------------------------------------------------------------------------------
 * Image prompts — the frozen CLIP vision tower (transformers CLIPVisionModel built at gill/models.py:78-96 and called by
 * GILLModel.get_visual_embs, gill/models.py:129-145: `self.visual_model(pixel_values).pooler_output`).
 * State-dict names are CLIPVisionModel's ("vision_model.embeddings.patch_embedding.weight",
 * "vision_model.encoder.layers.0.self_attn.q_proj.weight", "vision_model.pre_layrnorm.weight" (sic), ...).
 * ------------------------------------------------------------------------------------------ */
typedef struct gill_clip_config {
  int32_t image_size;         /* 224 */
  int32_t patch_size;         /* 14 (ViT-L/14) */
  int32_t hidden_size;        /* 1024 */
  int32_t num_layers;         /* 24 */
  int32_t num_heads;          /* 16 */
  int32_t intermediate_size;  /* 4096 */
  int32_t max_batch;
} gill_clip_config;
typedef struct gill_clip gill_clip;

int gill_clip_create(gill_clip** out, const gill_clip_config* cfg, const gill_tensor* weights, int n_weights);
void gill_clip_destroy(gill_clip* h);

/* pixel_values (B,3,S,S) fp32 (already resized / normalised)  ->  pooler_output (B, hidden) fp32. */
int gill_clip_forward(gill_clip* h, const float* pixel_values, int B, float* pooled_out, void* stream);

/* The image preprocessing in front of the tower (gill/utils.py:111-119: the CLIP feature extractor, called at gill/models.py:606-613):
 * bicubic resize of the shortest edge to `size` (the long edge becomes int(size * long / short)), centre crop to crop_size, x / 255,
 * (x - mean) / std with the CLIP constants.  The resize is Pillow's 8-bit BICUBIC resampler, integer for integer: 22-bit fixed-point
 * taps, the horizontal pass rounded and clipped to uint8 before the vertical one.
 *   packed     device, packed_bytes of uint8: n RGB images, HWC, of any sizes, anywhere in the buffer
 *   meta_host  HOST, n x 3 int64: byte offset, H, W of each image (edges 1 .. 32768)
 *   out        (n, 3, size, size) fp32;  out_u8 (n, size, size, 3) uint8 or NULL: the cropped pixels before normalisation
 *   workspace  device, 8-byte aligned, at least gill_clip_preprocess_workspace() bytes: tap tables and the uint8 intermediate
 * Only size == crop_size is built.  Two launches on `stream`; the tables are uploaded from a call-lifetime host buffer, so the call
 * waits for that copy (and for the work queued on the stream before it).  Nothing is allocated on the device. */
int gill_clip_preprocess_workspace(const int64_t* meta_host, int n, int size, int64_t* bytes_out);
int gill_clip_preprocess(const uint8_t* packed, int64_t packed_bytes, const int64_t* meta_host, int n, int size, int crop_size,
                         float* out, uint8_t* out_u8, void* workspace, int64_t workspace_bytes, void* stream);

/* HOST only: the tap tables of that resampler for the outputs first .. first + count - 1 of one axis resized in_size -> out_size:
 * xmin_out[i] the first input index, n_out[i] the tap count, k_out[i * k_stride + x] the fixed-point coefficients (zero past n_out[i]).
 * k_stride >= gill_clip_resize_ksize(in_size, out_size) = 2 ceil(2 max(in / out, 1)) + 1 (0 for sizes out of range). */
int gill_clip_resize_ksize(int in_size, int out_size);
int gill_clip_resize_taps(int in_size, int out_size, int first, int count, int32_t* xmin_out, int32_t* n_out, int32_t* k_out,
                          int k_stride);

/* ------------------------------------------------------------------------------------------
 * Text prompts — the CLIP text tower of the Stable Diffusion pipeline (transformers CLIPTextModel, `self.text_encoder` of
 * StableDiffusionPipeline: gill/custom_sd.py:305-309 and :353-357 read `text_encoder(input_ids)[0]`, i.e. last_hidden_state
 * AFTER final_layer_norm; _encode_prompt as a whole is gill/custom_sd.py:224-373, and scripts/preprocess_sd_embeddings.py:71
 * runs it over the captions the GILLMapper is trained to imitate).
 * State-dict names are those of the published checkpoint files ("text_model.embeddings.token_embedding.weight",
 * "text_model.embeddings.position_embedding.weight", "text_model.encoder.layers.0.self_attn.q_proj.weight",
 * "text_model.final_layer_norm.weight", ...); other entries ("text_model.embeddings.position_ids") are ignored.
 * ------------------------------------------------------------------------------------------ */
#define GILL_CLIP_TEXT_ACT_QUICK_GELU 0 /* x * sigmoid(1.702 x): SD-1.x (OpenAI ViT-L/14 text tower) */
#define GILL_CLIP_TEXT_ACT_GELU 1       /* exact (erf) GELU: SD-2.x (OpenCLIP ViT-H text tower as diffusers ships it) */
typedef struct gill_clip_text_config {
  int32_t vocab_size;         /* 49408 */
  int32_t hidden_size;        /* 768 (SD-1.5) / 1024 (SD-2.x); head dim hidden_size / num_heads must be 48/64/80/128/160 */
  int32_t num_layers;         /* 12 / 23 */
  int32_t num_heads;          /* 12 / 16 */
  int32_t intermediate_size;  /* 3072 / 4096 */
  int32_t max_positions;      /* 77: rows of position_embedding */
  int32_t hidden_act;         /* GILL_CLIP_TEXT_ACT_* */
  int32_t max_batch;          /* workspace sizing */
} gill_clip_text_config;
typedef struct gill_clip_text gill_clip_text;

int gill_clip_text_create(gill_clip_text** out, const gill_clip_text_config* cfg, const gill_tensor* weights, int n_weights);
void gill_clip_text_destroy(gill_clip_text* h);

/* text_encoder(input_ids)[0] (custom_sd.py:305-309): causal self-attention, no attention mask, LayerNorm eps 1e-5.
 *   ids (B,T) int32 on the DEVICE, every id in [0, vocab_size) (the caller validates: ids come from a CPU tokenizer),
 *   1 <= T <= max_positions, 1 <= B <= max_batch
 *   -> out_bf16 (B,T,hidden) bf16 (what gill_sd_denoise takes as cond / uncond) and / or out_f32 (B,T,hidden) fp32; either may be
 *   NULL, not both.  out_bf16 is the rounding of out_f32, written by the same pass.
 * Enqueued on `stream` only: no host synchronisation and no blocking copy, so the call can be captured into a graph. */
int gill_clip_text_forward(gill_clip_text* h, const int32_t* ids, int B, int T, void* out_bf16, float* out_f32, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stage 2 — GILLMapper = gill.layers.TextFcLayer(mode='gill_mapper').forward (layers.py:28-53).
 * State-dict names are TextFcLayer's ("fc.weight", "tfm.encoder.layers.0.self_attn.in_proj_weight",
 * "query_embs", "model.weight", ...).
 * ------------------------------------------------------------------------------------------ */
typedef struct gill_mapper gill_mapper;
typedef struct {
  int32_t in_dim;         /* 4096 (opt-6.7b) / 768 (opt-125m) */
  int32_t out_dim;        /* 768 */
  int32_t hidden_dim;     /* 512 */
  int32_t num_heads;      /* 4 */
  int32_t ffn_dim;        /* 2048 */
  int32_t num_enc_layers; /* 4 */
  int32_t num_dec_layers; /* 4 */
  int32_t num_input_tokens;  /* 8 */
  int32_t num_output_tokens; /* 77 */
  int32_t max_batch;
} gill_mapper_config;

int gill_mapper_create(gill_mapper** out, const gill_mapper_config* cfg, const gill_tensor* weights, int n_weights);
void gill_mapper_destroy(gill_mapper* h);
/* x (B,8,in_dim) bf16, input_embs (Be,8,in_dim) bf16 with Be in {1,B} (broadcast like torch)
 *   -> out (B,77,out_dim) fp32 */
int gill_mapper_forward(gill_mapper* h, const void* x_bf16, const void* input_embs_bf16, int B, int Be, float* out,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Stage 3 — Stable Diffusion UNet + PNDM/PLMS classifier-free-guidance loop.  Replaces
 * self.sd_pipe(prompt_embeds=..., guidance_scale=..., num_inference_steps=...) at
 * gill/models.py:730-731, whose driver is restated in-tree at gill/custom_sd.py:567-651.
 * State-dict names are diffusers UNet2DConditionModel's ("down_blocks.0.resnets.0.conv1.weight").
 * ------------------------------------------------------------------------------------------ */
typedef struct gill_unet gill_unet;
typedef struct {
  int32_t in_channels;          /* 4; 9 = 2 * out_channels + 1 for an inpainting UNet ([latents | mask | masked-image latents]); at most 14 */
  int32_t out_channels;         /* 4 */
  int32_t block_out_channels[4];/* 320,640,1280,1280 */
  int32_t layers_per_block;     /* 2 */
  int32_t cross_attention_dim;  /* 768 */
  int32_t num_heads;            /* 8 (SD-1.5's "attention_head_dim" is the head COUNT) */
  int32_t norm_num_groups;      /* 32 */
  int32_t sample_size;          /* 64 latent pixels per side */
  int32_t ctx_len;              /* 77 */
  int32_t max_batch;            /* largest UNet batch (2 x prompts with CFG) */
  int32_t heads_per_level[4];   /* all 0: num_heads at every level (SD-1.x); SD-2.x: 5,10,20,20 (head dim 64 everywhere) */
  int32_t v_prediction;         /* 0: the UNet predicts epsilon (SD-1.x, SD-2.1-base); 1: v (SD-2.1-768) */
  int32_t fp8_convs;            /* BASELINE configs[4] (no reference counterpart: the reference runs SD in fp16).  1: the ResnetBlock2D 3x3 convolutions
                                 * AND the GEGLU projections of the level 1-3 transformer blocks with fp8 (e4m3) activations and weights on the fp8
                                 * matrix instruction (csrc/conv_fp8.hip, csrc/linear_fp8.hip); 2: the convolutions only (the round-5 mode); 0: off
                                 * (bf16, the parity configuration) */
} gill_unet_config;

int gill_unet_create(gill_unet** out, const gill_unet_config* cfg, const gill_tensor* weights, int n_weights);
void gill_unet_destroy(gill_unet* h);

/* One UNet forward (custom_sd.py:633-638): sample (Bx,in_channels,L,L) fp32 NCHW (4; 9 on an inpainting handle), timesteps (Bx) fp32 HOST,
 * ctx (Bx,77,768) bf16 -> eps_out (Bx,4,L,L) fp32 NCHW. */
int gill_unet_forward(gill_unet* h, const float* sample, const float* timesteps_host, const void* ctx_bf16, int Bx,
                      float* eps_out, void* stream);

/* The whole denoise loop (custom_sd.py:607-651 with PNDMScheduler(skip_prk_steps, steps_offset=1,
 * scaled_linear 0.00085..0.012, 1000 train steps)):
 *   cond (B,77,768) bf16, uncond (n_uncond,77,768) bf16 with n_uncond == 1 (one negative embedding repeated over the batch,
 *   custom_sd.py:365-369) or == B (per-sample negative_prompt_embeds), latents0 (B,4,L,L) fp32 (already * init_noise_sigma=1)
 *   -> latents_out (B,4,L,L) fp32.  num_steps "inference steps" = num_steps+1 UNet calls of batch 2B.
 *   guidance <= 1 disables CFG (batch B, uncond ignored) like do_classifier_free_guidance.
 *   The loop is enqueued on a stream the handle owns, ordered after / before the caller's `stream` by events. */
int gill_sd_denoise(gill_unet* h, const void* cond_bf16, const void* uncond_bf16, int n_uncond, const float* latents0, int B,
                    int num_steps, float guidance, float* latents_out, void* stream);

/* The same loop under another sampler (the reference's pipeline is written against KarrasDiffusionSchedulers, custom_sd.py:86).  Tables follow
 * diffusers 0.17.1 with scaled_linear betas 0.00085..0.012 over 1000 train steps; DPM-Solver++ is (2M): solver_order 2, midpoint,
 * lower_order_final, no thresholding, no Karras sigmas; Euler has s_churn 0. */
typedef struct {
  int32_t kind;             /* 0 pndm, 1 ddim, 2 dpmsolver++ (2M), 3 euler, 4 euler_ancestral */
  int32_t steps_offset;     /* pndm / ddim; 1 for SD */
  int32_t set_alpha_to_one; /* pndm / ddim; 0 for SD */
  float eta;                /* ddim */
} gill_sd_sampler;

/* gill_sd_denoise with a sampler; kind 0 (steps_offset 1, set_alpha_to_one 0) is gill_sd_denoise itself, bit for bit.  The sampler multiplies
 * latents0 by its init_noise_sigma itself (custom_sd.py:472): pass the unit-variance draw.  num_steps >= 1 (pndm: >= 2) UNet calls
 * (pndm: num_steps + 1).  noise: (ncalls,B,4,L,L) fp32 on the device, unit variance, row i read by call i — required when a row of the table has
 * c_n != 0 (ddim with eta > 0, euler_ancestral), otherwise never read and may be NULL.  v-prediction comes from the handle's configuration. */
int gill_sd_denoise_ex(gill_unet* h, const gill_sd_sampler* sampler, const void* cond_bf16, const void* uncond_bf16, int n_uncond,
                       const float* latents0, int B, int num_steps, float guidance, float* latents_out, const float* noise, void* stream);

/* The tables gill_sd_denoise_ex runs on, for tests and callers that must know the number of calls (host arrays, no GPU needed).  Returns the
 * number of UNet calls (<= num_steps + 1), negative on invalid arguments.  Every output may be NULL.  timesteps_out: one float per call (Euler's are
 * fractional).  rows_out: GILL_SD_ROW_DOUBLES doubles per call, the fp32 values the device reads, widened:
 *   [0] mode  [1] slot_new  [2] s1  [3] s2  [4] s3  [5] in_scale  [6] p_x  [7] p_e  [8] c_x  [9] c_0  [10] c_1  [11] c_n
 * With e the guided model output, x the latents and ring[] the stored history:
 *   mode -1 (every kind but pndm):  m = p_x x + p_e e;  if slot_new >= 0: ring[slot_new] = m;
 *                                   x_next = c_x x + c_0 m + c_1 ring[s1] + c_n noise[call]      (the UNet sees in_scale * x)
 *   mode 0..4 (pndm; v-prediction is folded into c_x, c_0):  x_next = c_x x' + c_0 e'  with
 *     0: e' = e, x' = x, saved = x, ring[slot_new] = e          1: e' = (e + ring[s1]) / 2, x' = saved
 *     2..4: ring[slot_new] = e, then e' = (3 e - ring[s1]) / 2;  (23 e - 16 ring[s1] + 5 ring[s2]) / 12;
 *           (55 e - 59 ring[s1] + 37 ring[s2] - 9 ring[s3]) / 24;  x' = x */
#define GILL_SD_ROW_DOUBLES 12
int gill_sd_schedule(const gill_sd_sampler* sampler, int v_prediction, int num_steps, float* timesteps_out, double* init_noise_sigma_out,
                     double* rows_out);

/* Image-to-image: the loop started part-way.  `start` counts sampler steps, 0 <= start < num_steps (negative return otherwise); start == 0 gives
 * gill_sd_schedule's tables bit for bit.  The loop then begins at the timestep t_s of step `start` of the full schedule:
 *   ddim, euler, euler_ancestral: the tail of the full table (num_steps - start calls);
 *   dpmsolver++: the tail with its first row rebuilt as a first-order step — the solver starts with an empty history, as diffusers' scheduler does
 *     when it is handed the sliced timestep list; the ring slots of the following rows stay those of the full table;
 *   pndm: the PLMS warm-up pair replayed at t_s — timesteps t_s, t_s - D, t_s - D, t_s - 2D, ... (D = 1000 / num_steps), num_steps - start + 1
 *     calls.  A DELIBERATE difference from diffusers 0.17's img2img pipeline, which slices the already-duplicated list [t_0, t_1, t_1, t_2, ...]
 *     at `start`: for start >= 2 PNDMScheduler.step_plms then takes the first timestep it sees for the warm-up and from the third call on
 *     evaluates the model one grid step ahead of the latents.  Here the warm-up is what a fresh num_steps-grid run from t_s would do.
 * add_noise_out (optional, 2 doubles): the pair (a, b) of x_start = a * init_latents + b * init_noise, the schedulers' add_noise() at the
 * first timestep: pndm, ddim, dpmsolver++ (sqrt(abar_t), sqrt(1 - abar_t)); euler, euler_ancestral (1, sigma of the first call).  The other outputs as
 * gill_sd_schedule (init_noise_sigma_out: unchanged by start — not used by a loop that starts from an image). */
int gill_sd_schedule_from(const gill_sd_sampler* sampler, int v_prediction, int num_steps, int start, float* timesteps_out,
                          double* init_noise_sigma_out, double* rows_out, double* add_noise_out);
/* gill_sd_denoise_ex from step `start`: the first kernel forms x_start = a * init_latents + b * init_noise (both (B,4,L,L) fp32, init_latents the
 * scaled VAE latents of the image, init_noise a unit-variance draw) in place of latents0 * init_noise_sigma; noise: as gill_sd_denoise_ex, one row
 * per call of THIS table.  The captured step, the step counter and the time-embedding table are those of gill_sd_denoise_ex. */
int gill_sd_denoise_from(gill_unet* h, const gill_sd_sampler* sampler, const void* cond_bf16, const void* uncond_bf16, int n_uncond,
                         int start, const float* init_latents, const float* init_noise, int B, int num_steps, float guidance,
                         float* latents_out, const float* noise, void* stream);

/* Inpainting: repaint where the mask is 1, keep the image where it is 0.  Mask values are in [0,1]; a pixel counts as repaint when it is >= 0.5.
 * gill_sd_inpaint_prepare (device pointers, one kernel on `stream`, no synchronisation): image (B,3,H,W) fp32 in [-1,1], mask (Bm,1,H,W) fp32 with
 * Bm == 1 (one mask for every sample) or Bm == B; H, W multiples of 8 -> masked_image_out (B,3,H,W) = image where mask < 0.5, else 0, and
 * latent_mask_out (B,1,H/8,W/8) in {0,1} = (mask[b][0][8y][8x] >= 0.5): what torch's nearest interpolation to 1/8 size gives, one channel. */
int gill_sd_inpaint_prepare(const float* image, const float* mask, int B, int Bm, int H, int W, float* masked_image_out, float* latent_mask_out,
                            void* stream);
/* The blend table of gill_sd_inpaint (host arrays, no GPU needed).  keep_out (optional): [ncalls][2] doubles, the fp32 values the device reads,
 * widened: row i is the schedulers' add_noise pair (ka, kb) at the noise level the latents have AFTER call i of gill_sd_schedule_from(...,
 * start)'s table, so that ka * init_latents + kb * init_noise is the image at that level.  Rows i < ncalls - 1 are the pair at the timestep of call
 * i + 1: ddim, dpmsolver++ (sqrt(abar_t), sqrt(1 - abar_t)); euler, euler_ancestral (1, sigma of call i + 1); pndm (sqrt(abar_t), sqrt(1 - abar_t))
 * at timestep i + 1 of the replayed warm-up list, so rows 0 and 1 are equal (both calls leave the latents at t_s - D).  The last row is (1, 0): the
 * kept region ends as the clean image latents.  Returns ncalls, negative on the arguments gill_sd_schedule_from refuses. */
int gill_sd_inpaint_keep(const gill_sd_sampler* sampler, int v_prediction, int num_steps, int start, double* keep_out);
/* gill_sd_denoise_from with a mask: the same start x_start = a * init_latents + b * init_noise at step `start`, the same tables, step counter and
 * noise rows.  latent_mask (B,1,L,L) fp32, 1 = repaint (gill_sd_inpaint_prepare's output; one plane per sample, broadcast over the channels).
 * The handle decides what masked_latents must be, and anything else is an error that says which:
 *   masked_latents == NULL, handle with in_channels == out_channels (every text-to-image checkpoint) — BLEND mode: after the sampler step of call
 *     i one more kernel sets latents = m * latents + (1 - m) * (ka[i] * init_latents + kb[i] * init_noise), (ka, kb) = gill_sd_inpaint_keep's row i;
 *   masked_latents (B,4,L,L) fp32 = the scaled VAE latents of the masked image, handle with in_channels == 2 * out_channels + 1 — CONCAT mode: no
 *     blend; the UNet input of every call is [in_scale * latents (4) | latent_mask (1) | masked_latents (4)] per sample, in both CFG halves.
 * Latents, sampler state, noise and latents_out keep out_channels channels in both modes.  init_latents, init_noise, latent_mask and
 * masked_latents are copied into the handle before the loop: the captured step (one per mode, apart from the graphs of gill_sd_denoise*, which
 * are unchanged) serves every call.  gill_sd_denoise* on a concat-mode handle is refused. */
int gill_sd_inpaint(gill_unet* h, const gill_sd_sampler* sampler, const void* cond_bf16, const void* uncond_bf16, int n_uncond, int start,
                    const float* init_latents, const float* init_noise, const float* latent_mask, const float* masked_latents, int B,
                    int num_steps, float guidance, float* latents_out, const float* noise, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stage 3b — VAE decode of the final latents.  Replaces StableDiffusionPipeline.decode_latents
 * (gill/custom_sd.py:385-392: latents / 0.18215 -> vae.decode -> (x/2+0.5).clamp(0,1)) and the uint8 conversion
 * of numpy_to_pil (custom_sd.py:660-661).  State-dict names are diffusers AutoencoderKL's
 * ("post_quant_conv.weight", "decoder.up_blocks.2.resnets.0.conv1.weight", ...).
 * ------------------------------------------------------------------------------------------ */
typedef struct gill_vae gill_vae;
typedef struct {
  int32_t latent_channels;       /* 4 */
  int32_t out_channels;          /* 3 */
  int32_t block_out_channels[4]; /* 128,256,512,512 */
  int32_t layers_per_block;      /* 2 */
  int32_t norm_num_groups;       /* 32 */
  int32_t latent_size;           /* 64 -> 512x512 pixels */
  float scaling_factor;          /* 0.18215 (hard-coded at custom_sd.py:387) */
  int32_t max_batch;
} gill_vae_config;

int gill_vae_create(gill_vae** out, const gill_vae_config* cfg, const gill_tensor* weights, int n_weights);
void gill_vae_destroy(gill_vae* h);
/* latents (B,4,L,L) fp32 -> image_f32 (B,3,8L,8L) fp32 in [-1,1] (vae.decode(...).sample; may be NULL) and/or
 * image_u8 (B,8L,8L,3) uint8 = round(255 * clamp(x/2+0.5, 0, 1)) (may be NULL). */
int gill_vae_decode(gill_vae* h, const float* latents, int B, float* image_f32, uint8_t* image_u8, void* stream);
/* The encoder half (AutoencoderKL.encode(image).latent_dist, then * scaling_factor): present in the handle when the weight table holds
 * "encoder.conv_in.weight" (then all of encoder.* and quant_conv.* must be there); a decoder-only handle allocates nothing for it and refuses
 * this call.  image (B,3,8L,8L) fp32 NCHW in [-1,1]; noise (B,latent_channels,L,L) fp32 unit variance, or NULL for the posterior mode
 *   -> latents_out (B,latent_channels,L,L) = scaling_factor * (mean + exp(0.5 * logvar) * noise)      (NULL noise: scaling_factor * mean)
 *      moments_out (B,2*latent_channels,L,L) = [mean | clamp(logvar, -30, 20)], unscaled; may be NULL. */
int gill_vae_encode(gill_vae* h, const float* image, int B, const float* noise, float* latents_out, float* moments_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Retrieval — the image-retrieval half of GILL.generate_for_images_and_texts (gill/models.py:671-696): ret_emb / ||ret_emb|| ->
 * scores = emb_matrix @ ret_emb.T -> scores[seen] -= 1000 -> topk(3), and the index preparation of load_gill (gill/models.py:895-900):
 * emb_matrix = exp(logit_scale) * m / ||m||.  Here the matrix lives on the device in a handle (bf16, in the A-operand order of the
 * 16x16x32 bf16 matrix instruction: csrc/retrieval.hip), and one fused pass scores up to 16 queries against every row and keeps the top k.
 * The full score vector is never written.
 * DIVERGENCES from the reference, all deliberate: a zero row (and a zero query under normalize) stays zero where the reference's division
 * gives NaN; the ranking is on the fp32 accumulated scores (the reference rounds the score vector to the matrix's dtype first) and a tie goes
 * to the LOWER row index (torch.topk promises no order among equals); a row listed several times in `exclude` is penalised once.
 * ------------------------------------------------------------------------------------------ */
typedef struct gill_ret_index gill_ret_index;

/* An empty index of `capacity` rows of `dim` columns: dim a multiple of 8, at most 1024; 1 <= capacity < 2^31 - 1.  Host only: the device memory
 * (capacity rounded up to 16 rows x dim rounded up to 32 columns of bf16, plus a workspace of at most 16 MiB) is allocated by the first add / search. */
int gill_ret_index_create(gill_ret_index** out, int dim, int64_t capacity);
void gill_ret_index_destroy(gill_ret_index* h);
/* Append rows (n, dim) of dtype GILL_DTYPE_* (device pointer, 16-byte aligned); models.py:895-900 with normalize = 1: every row becomes
 * scale * row / ||row||_2, computed in fp32 and rounded once to bf16 (a zero row stays zero).  normalize = 0: the rows rounded to bf16 as they
 * are (scale unused).  An error, with nothing written, when size + n would pass the capacity. */
int gill_ret_index_add(gill_ret_index* h, const void* rows, int dtype, int64_t n, int normalize, float scale, void* stream);
/* Rows held (-1 for a null handle).  Host only. */
int64_t gill_ret_index_size(const gill_ret_index* h);
/* Rows [first, first + n) as stored -> out (n, dim) bf16 row-major (device pointer, 16-byte aligned). */
int gill_ret_index_rows(gill_ret_index* h, int64_t first, int64_t n, void* out_bf16, void* stream);
/* models.py:671-696.  queries (Q, dim) fp32 on the device (16-byte aligned), any Q >= 1 (one pass over the matrix per 16 queries); normalize = 1:
 * each query is divided by its fp32 L2 norm, then rounded to bf16; 0: rounded as it is.  Scores are fp32 sums of bf16 products.
 * exclude (Q, E) int64 on the device or NULL, E <= 64, -1 = empty slot: a listed row competes with score - penalty (it is not removed:
 * `scores[seen_idx] -= 1000`, :688-689) and is reported with it.  -> scores_out (Q, k) fp32, idx_out (Q, k) int64, 1 <= k <= 32: the exact top k
 * by (score descending, row index ascending); when k > size the trailing slots hold index -1 and score -inf.  Scores are assumed finite.
 * Three launches per 16 queries on `stream` (five from 16384 rows on: the first 1/64 of the rows is searched first and its k-th score is
 * the floor the rest starts its filter from), no host synchronisation; the partial lists live in the handle (one search at a time). */
int gill_ret_index_search(gill_ret_index* h, const float* queries, int Q, int normalize, int k, const int64_t* exclude, int E, float penalty,
                          float* scores_out, int64_t* idx_out, void* stream);
/* How a search of the index as it stands splits the rows (host only, for tests): rows below *first_row belong to the prefix pass; list j of the
 * *nlists of the main pass scans rows *first_row + [j, j + 1) * *rows_per_list, one wave each.  The result never depends on it.  Any output may
 * be NULL. */
int gill_ret_index_slabs(const gill_ret_index* h, int64_t* first_row, int* nlists, int64_t* rows_per_list);

/* PNDM schedule known-answers for tests (host arrays): timesteps_out must hold num_steps+1 ints;
 * returns the number written.  alphas_cumprod_out (optional) must hold 1000 doubles. */
int gill_pndm_schedule(int num_steps, int32_t* timesteps_out, double* alphas_cumprod_out);
/* Exclusive-device contract of the UNet engine (round 6).  Some of its 3x3 convolutions finish the GroupNorm that consumes them inside their own
 * launch: their workgroups wait for each other on arrival counters, which is deadlock-free only while the handle's stream has the device's CUs to
 * itself (one process per GPU, as DESIGN.md section 5 deploys it; kernels of other streams that do not themselves wait only delay it).  Two such
 * launches running side by side (two processes sharing one GPU, two handles on two streams) can starve each other: the waits are bounded, a
 * workgroup that gives up NaN-poisons its outputs and counts itself.  gill_unet_forward / gill_sd_denoise fail with -5 when the count is non-zero
 * on entry (and clear it); this function reads and clears it on demand (synchronous small copy; < 0 on a HIP error).  GILL_GEMM_COOP=0 in the
 * environment turns the in-kernel finishes off (every GroupNorm a launch of its own, the round-5 dataflow: -0.6 % on the loop). */
int gill_coop_timeouts(void);

/* ------------------------------------------------------------------------------------------
 * Operator-level entry points (the kernels the three stages are built from), exported so the
 * parity tests can pin each against the CPU oracle.  All bf16 unless noted.
 * ------------------------------------------------------------------------------------------ */
/* C[M,N] = act(alpha * A[M,K] . W[N,K]^T + bias[N] + resid[M,N]); act: 0 none 1 relu 2 gelu(erf) 3 silu.
 * out_f32: bit 0: C is fp32 instead of bf16; bit 1: resid is fp32 (as the OPT / CLIP engines keep their residual stream).  splitk: 0 = auto, n > 1 = forced n-way split; < 0 = the general row-major tiles even for the
 * weight-streaming shapes (N * K >= 4 Mi) that otherwise run on a 64 x 64-blocked copy of W — the STREAM64 tile up to 256 rows, the general tiles reading
 * the blocked layout above — (-1: auto split, -n: n ways).
 * Split-K launches share one grow-only workspace owned by the library: one caller at a time (as everywhere on this path). */
int gill_op_gemm(const void* A, const void* W, const float* bias, const void* resid, void* C, int M, int N, int K,
                 float alpha, int act, int out_f32, int splitk, void* stream);
/* GEGLU projection: W (2*inner, K) in diffusers order [value rows | gate rows], bias (2*inner) ->
 * C (M, inner) = (A.Wv^T + bv) * gelu(A.Wg^T + bg) */
int gill_op_geglu(const void* A, const void* W, const float* bias, void* C, int M, int inner, int K, void* stream);
/* 3x3 pad-1 convolution over NHWC: x1 (B,IH,IW,C1) [++ x2 (B,IH,IW,C2) channel-concat], w OIHW fp32 (Cout,C1+C2,3,3),
 * stride 1|2, ups=1 -> nearest 2x upsample first.  rowvec (B,Cout) fp32 optional per-sample bias; resid NHWC optional. */
int gill_op_conv3x3(const void* x1, int C1, const void* x2, int C2, const float* w_oihw, const float* bias,
                    const float* rowvec, const void* resid, void* y, int B, int IH, int IW, int Cout, int stride, int ups,
                    int splitk, void* stream);
/* gill_op_conv3x3 with the gather's origin shift: pad_shift = 1 (stride 2, even IH and IW, no upsample) is diffusers' Downsample2D with
 * padding 0 — F.pad(x, (0, 1, 0, 1)) then conv(stride 2, pad 0): output (oy, ox) reads rows 2 oy .. 2 oy + 2, columns 2 ox .. 2 ox + 2, zero
 * past the bottom / right edge.  pad_shift = 0 is gill_op_conv3x3 itself. */
int gill_op_conv3x3_ex(const void* x1, int C1, const void* x2, int C2, const float* w_oihw, const float* bias,
                       const float* rowvec, const void* resid, void* y, int B, int IH, int IW, int Cout, int stride, int ups,
                       int pad_shift, int splitk, void* stream);
/* 3x3 convolution (stride 1, pad 1) + the GroupNorm (+ SiLU) that consumes it, without a GroupNorm launch where the geometry allows (diffusers
 * ResnetBlock2D: conv1 -> norm2 -> silu, conv2 -> the next block's norm; reference call site gill/custom_sd.py:633-638):
 * y_raw (optional, may be NULL) = conv(x) + bias + rowvec[b] + resid, y_norm = [silu](GroupNorm(y_raw)).
 * x (B,H,W,Cin) bf16 NHWC, w (Cout,Cin,3,3) fp32, rowvec (B,Cout) fp32 optional, gamma / beta (Cout) fp32.
 * splitk >= 2: H * W in {64, 256}, Cout % 80 == 0, Cout / groups a multiple of 4 that divides 80; the normalisation runs in the split-K reducer
 *   launch; coop is ignored.
 * splitk == 1: coop = 1: in the convolution's epilogue (rows per sample a multiple of the 128- / 256-row tile, B * H * W % 256 == 0, Cout % 160 == 0,
 *   grid <= CUs; an error elsewhere); coop = 0: convolution with fused statistics + a GroupNorm-apply launch (the reference dataflow).
 * ss_out (optional; splitk == 1 && coop only): the scale | shift table [B][2][Cout] fp32 (y = x * scale + shift); y_norm may then be NULL.
 * Synchronises. */
int gill_op_conv3x3_gn(const void* x, const float* w_oihw, const float* bias, const float* rowvec, const void* resid, const float* gamma,
                       const float* beta, int groups, float eps, int silu, void* y_raw, void* y_norm, float* ss_out, int B, int H, int W,
                       int Cin, int Cout, int splitk, int coop, void* stream);
/* conv3x3 (stride 1, pad 1) of x1 ++ x2 plus a fused 1x1 convolution of xs1 ++ xs2 (ResnetBlock2D.conv2 + conv_shortcut as one
 * implicit GEMM): y (B,IH,IW,Cout) bf16 NHWC; w_oihw (Cout, C1+C2, 3, 3) fp32, w_sc (Cout, CS1+CS2) fp32.  Synchronises. */
int gill_op_conv3x3_shortcut(const void* x1, int C1, const void* x2, int C2, const float* w_oihw, const float* bias,
                             const void* xs1, int CS1, const void* xs2, int CS2, const float* w_sc, void* y, int B, int IH, int IW,
                             int Cout, int splitk, void* stream);
/* softmax(scale * q k^T [+causal]) v over token-major q (B,nq,H*d), k/v (B,nkv,H*d) -> o (B,nq,H*d) */
int gill_op_attention(const void* q, const void* k, const void* v, void* o, int B, int H, int nq, int nkv, int d,
                      float scale, int causal, void* stream);
int gill_op_layernorm(const void* x, int x_f32, const float* gamma, const float* beta, void* y_bf16, int rows, int C,
                      float eps, void* stream);
int gill_op_groupnorm(const void* x1, int C1, const void* x2, int C2, int B, int HW, int groups, const float* gamma,
                      const float* beta, float eps, int silu, void* y, void* stream);

/* Fused GroupNorm statistics, producer side: a GEMM / 3x3 convolution launched as the engines launch it with fused statistics, returning
 * what it filed.  gn_stats: fp32 partial sums {sum, sum of squares} of the bf16 OUTPUT tensor in bins of `bin` channels (bin must divide
 * Cout / N and pass the launcher's tile rules; an error otherwise), laid out [B][*nslab][Cout / bin][2]; the caller sizes the buffer for
 * 16-row slabs (B * rows / 16 * (Cout / bin) * 2 floats, rows = output pixels per sample, a multiple of 64) and only the first
 * B * *nslab * (Cout / bin) * 2 floats are written.  *slab_rows = rows per partial, *nslab = rows / *slab_rows.  Slab layout:
 *   unsplit (splitk <= 1), stride-1 forms and the plain GEMM: slab j of sample b = output rows [64 j, 64 j + 64) of the sample, row-major
 *     pixel order (*slab_rows = 64);
 *   four-tap upsample form (ups = 1: nearest-2x upsample + conv as four 2x2-tap kernels on the SOURCE grid, one per output parity class
 *     cls = 2 (oy % 2) + (ox % 2)): slab index = cls * (IH * IW / 64) + j, holding the output pixels (2 sy + cls / 2, 2 sx + cls % 2) of the
 *     source pixels sy * IW + sx in [64 j, 64 j + 64) (*slab_rows = 64, *nslab = 4 IH IW / 64; IH * IW a multiple of 64);
 *   split-K (splitk >= 2): the reducer files them, slab j = output rows [R j, R j + R) with R = *slab_rows = 64 where the reducer's grid is
 *     large (ceil(N / block width) * ceil(M / 64) >= 1024 blocks), else 16.
 * gill_op_conv3x3_gn_stats: 3x3 / pad 1 / stride 1 convolution of x1 (B,IH,IW,C1) [++ x2 (…,C2)], w (Cout,C1+C2,3,3) fp32, optional bias (Cout),
 *   rowvec (B,Cout), resid (B,IH,IW,Cout) bf16; xs1 (…,CS1) [++ xs2 (…,CS2)] with w_sc (Cout,CS1+CS2) fp32: the fused 1x1 shortcut segment
 *   (then no rowvec / resid); ups = 1: the four-tap upsample form (y (B,2IH,2IW,Cout); no rowvec / resid / shortcut).
 * gill_op_gemm_gn_stats: C (M,N) bf16 = act(A (M,K) . W (N,K)^T + bias + resid (M,N)), M = samples x rows_per_batch, ldc = N; act as gill_op_gemm
 *   (the time-embedding style SiLU GEMM with statistics: the one launch that runs the two-wave 64 x 128 tile with an activation).
 * Synchronise.  For the operator tests. */
int gill_op_conv3x3_gn_stats(const void* x1, int C1, const void* x2, int C2, const float* w_oihw, const float* bias, const float* rowvec,
                             const void* resid, const void* xs1, int CS1, const void* xs2, int CS2, const float* w_sc, void* y, float* gn_stats,
                             int bin, int B, int IH, int IW, int Cout, int ups, int splitk, int* slab_rows, int* nslab, void* stream);
int gill_op_gemm_gn_stats(const void* A_bf16, const void* W_bf16, const float* bias, const void* resid_bf16, void* C_bf16, float* gn_stats, int bin,
                          int M, int N, int K, int rows_per_batch, int splitk, int act, int* slab_rows, int* nslab, void* stream);
/* ... consumer side: GroupNorm (+ SiLU) of x1 (B,HW,C1) [++ x2 (B,HW,C2)] from caller-supplied partials, never reading the tensors for
 * statistics.  stats1 [B][nslab1][C1 / bin1][2] covers the channels of x1, stats2 [B][nslab2][C2 / bin2][2] those of x2 (NULL when C2 == 0);
 * group boundaries must fall on bin boundaries of the block that holds them (an error otherwise); at most 128 bins per block; any partial
 * counts (more than 64 go through an out-of-place totals pass; the partials themselves are never modified).  y (B,HW,C1+C2) bf16; ss_out
 * (optional, single-source only): the scale | shift table [B][2][C1] fp32 (y = x * scale + shift) is written INSTEAD of y.  out8_scale > 0: y is
 * (B,HW,C1+C2) e4m3 bytes holding fp8(out8_scale * value), the A operand of the fp8 convolution (0: bf16).  Synchronises. */
int gill_op_groupnorm_from_stats(const void* x1, int C1, const void* x2, int C2, int B, int HW, int groups, const float* gamma, const float* beta,
                                 float eps, int silu, const float* stats1, int bin1, int nslab1, const float* stats2, int bin2, int nslab2,
                                 void* y, float* ss_out, float out8_scale, void* stream);

/* The VAE mid block's single-head attention behind its GroupNorm, launched as the engine launches it (diffusers AutoencoderKL
 * mid_block.attentions.0 without group_norm): out (B*HW, C) bf16 = to_out(softmax(to_q(n) to_k(n)^T / sqrt(C)) to_v(n)) + resid.  n (B*HW, C)
 * bf16: the normalised input; resid (B*HW, C) bf16 or NULL; wqkv (3C, C) bf16 = to_q | to_k | to_v rows, bqkv (3C) fp32; wo (C, C) bf16,
 * bo (C) fp32.  P_out (B, HW, HW) bf16 or NULL: every image's probabilities as stored (NULL: one score buffer reused by every image, as in
 * the engine).  splits: three ints, the split-K factors used by the QKV, S = Q K^T and O = P V GEMMs (the engine's rule under its 16 Mi-float
 * workspace).  HW and C must be multiples of 64 (an error otherwise).  Synchronises.  For the operator tests. */
int gill_op_vae_attention(const void* n_bf16, const void* resid_bf16, const void* wqkv_bf16, const float* bqkv, const void* wo_bf16,
                          const float* bo, void* out_bf16, void* P_out_bf16, int B, int HW, int C, int* splits, void* stream);
/* In-place softmax over the rows of s (rows, n) bf16, the VAE attention's kernel with the engine's launch geometry.  n must be a multiple of
 * 8 (an error otherwise: nothing is launched).  Synchronises. */
int gill_op_row_softmax(void* s_bf16, int rows, int n, void* stream);

/* The feed-forward sub-block of a level-0 (C = 320) transformer block + proj_out + outer residual as one kernel (csrc/ffn.hip):
 * out = proj_out(ff2(geglu(ff1(LN(t)))) + t) + resid on natural (diffusers-layout) operands; gn_stats (optional): GroupNorm partial sums
 * of the output, [(b * rows_per_batch / 64 + slab) * 64 + bin][2], bins of 5 channels.  Replaces, inside gill_unet_forward, the
 * BasicTransformerBlock.ff call + Transformer2DModel.proj_out of diffusers (reference call site: gill/custom_sd.py:633-638).
 * o2 / Wo / bo2 (optional, all or none): t := t + attn2.to_out(o2) first, inside the kernel (o2 (M, 320) = the cross-attention output,
 * Wo (320, 320), bo2 (320)) — the form the UNet engine runs. */
int gill_op_ffn_fused(const void* t_bf16, const float* ln_g, const float* ln_b, const void* W1_bf16, const float* b1,
                      const void* W2_bf16, const float* b2, const void* Wp_bf16, const float* bp, const void* resid_bf16,
                      void* out_bf16, float* gn_stats, int M, int rows_per_batch, const void* o2_bf16, const void* Wo_bf16,
                      const float* bo2, void* stream);
/* The same with the caller's LayerNorm row-sum planes, as the engine passes the ones its producing GEMM filed: ln_stats (nullable: the entry
 * then forms one plane itself, as gill_op_ffn_fused) [ln_planes][R][2] fp32 {sum, sum of squares} of the rows of t, added in plane order,
 * R = ln_rows ? ln_rows : M; rows m >= R read the sums of row m - R (M <= 2 ln_rows).  Not together with o2 (that form takes the
 * statistics in registers): an error. */
int gill_op_ffn_fused_ex(const void* t_bf16, const float* ln_g, const float* ln_b, const void* W1_bf16, const float* b1,
                         const void* W2_bf16, const float* b2, const void* Wp_bf16, const float* bp, const void* resid_bf16,
                         void* out_bf16, float* gn_stats, int M, int rows_per_batch, const void* o2_bf16, const void* Wo_bf16,
                         const float* bo2, const float* ln_stats, int ln_planes, int ln_rows, void* stream);

/* BASELINE configs[4] (not a reference function): the GEGLU projection of a BasicTransformerBlock (diffusers ff.net.0; reference call site
 * gill/custom_sd.py:633-638) on CDNA4's fp8 matrix instruction — out (M, inner) bf16 = h * gelu(g), [h | g] = LayerNorm(t; ln_g, ln_b) W^T + b with
 * t (M, C) bf16, W (2 inner, C) bf16 in diffusers order [value rows | gate rows], b (2 inner) fp32; activations and weights quantised to e4m3 exactly as
 * the engine's fp8 mode does (per-row weight scales, fp8(16 * LNhat(t))).  inner % 16 == 0, C % 128 == 0.  Synchronises. */
int gill_op_geglu_fp8(const void* t, const float* ln_g, const float* ln_b, const void* W, const float* b, void* out, int M, int inner, int C,
                      void* stream);
/* The two projections around norm1 / norm2 of a level-0 (C = 320, 8 heads of 40) transformer block as one kernel (csrc/lnproj.hip), on
 * natural (diffusers-layout) operands.  mode 0: t = proj_in(x); [q | k | v] = [to_q; to_k; to_v](LN(t)) (W2 = the three weights stacked,
 * (960, 320)).  mode 1: t += to_out(x) + b1 (in place, x = the attention output); q = to_q(LN(t)) (W2 (320, 320)).  Outputs in the
 * attention kernels' layouts: q, k [B][8][hw_pad][48] bf16 (q pre-scaled by log2(e) / sqrt(40)), vt [B][8][64][hw_pad] (row 48 = 1);
 * hw_pad = HW rounded up to 32; B * HW a multiple of 128.  Replaces, inside gill_unet_forward, Transformer2DModel.proj_in + norm1 +
 * attn1.to_q/k/v, resp. attn1.to_out + residual + norm2 + attn2.to_q of diffusers (reference call site: gill/custom_sd.py:633-638).
 * Synchronises. */
int gill_op_lnproj(int mode, const void* x_bf16, void* t_bf16, const void* W1_bf16, const float* b1, const float* ln_g, const float* ln_b,
                   const void* W2_bf16, void* q_bf16, void* k_bf16, void* vt_bf16, int B, int HW, void* stream);
/* The same with the block's GroupNorm applied to the rows of x as the kernel loads them, the form the UNet engine runs where a sample is
 * whole 128-row tiles: gn_ss (nullable) [B][2][320] fp32 = per sample the scale row, then the shift row; x := bf16(x * scale + shift).
 * With a table: mode 0 and HW % 128 == 0 only (an error otherwise: nothing is launched). */
int gill_op_lnproj_ex(int mode, const void* x_bf16, void* t_bf16, const void* W1_bf16, const float* b1, const float* ln_g, const float* ln_b,
                      const void* W2_bf16, void* q_bf16, void* k_bf16, void* vt_bf16, int B, int HW, const float* gn_ss, void* stream);

/* attn2 (cross-attention) of a UNet transformer block with heads of 80..160 features, as the two GEMMs on per-sample weights the engine
 * runs at UNet levels 1-3 (csrc/xf_weights.hip "XALG"): K and V are linear in the prompt context, so qs (g o Wq_h)^T Wk_h and Wo_h Wv_h are
 * folded at load, multiplied by ctx once per prompt, and each UNet call computes P = softmax(LN(t) Mq_b^T) and out = t + P Wo_b^T + bo.
 * Operands in diffusers layout: t (B * HW, C) bf16, norm2 gain / bias (C) fp32, to_q / to_out.0 weights (C, C) bf16, to_k / to_v (C, E)
 * bf16, to_out.0 bias (C) fp32, ctx (B, ctx_len <= 80, E) bf16 -> out (B * HW, C) bf16; P_bf16 (optional, B * HW x 80 H): the softmax
 * weights, key j of head h at column 80 h + j.  Replaces norm2 + CrossAttention(attn2) + residual of diffusers' BasicTransformerBlock inside
 * gill_unet_forward (reference call site: gill/custom_sd.py:633-638).  Synchronises. */
int gill_op_cross_attention_folded(const void* t_bf16, const float* ln_g, const float* ln_b, const void* Wq_bf16, const void* Wk_bf16,
                                   const void* Wv_bf16, const void* Wo_bf16, const float* bo, const void* ctx_bf16, void* out_bf16,
                                   void* P_bf16, int B, int HW, int C, int H, int ctx_len, int E, void* stream);

/* The folded-LayerNorm chain of UNet levels 1-3 (csrc/unet.hip xf(): norm1 / norm2 / norm3 never run as kernels), one GEMM each.
 * Producer: T (M, N) bf16 = [A (M, K1) | A2 (M, K - K1)] . W (N, K)^T + bias + resid (resid may be T itself), as the engine's linear() launches
 * it with GemmArgs::row_stats set; planes ([*nplanes][M][2] fp32, room for planes_cap planes) = {sum, sum of squares} of every stored row over the
 * columns of each plane, *nplanes = what gemm_row_planes() reports for the launch.  A2 null when K1 == K.  splitk: 0 = the engine's heuristic,
 * 1 = unsplit (planes from the GEMM epilogue), n > 1 = forced (planes from the split-K reducer).  Synchronises. */
int gill_op_linear_rowstats(const void* A_bf16, const void* A2_bf16, int K1, const void* W_bf16, const float* bias, const void* resid_bf16,
                            void* T_bf16, float* planes, int planes_cap, int* nplanes, int M, int N, int K, int splitk, void* stream);
/* Consumer: LayerNorm(T; ln_g, ln_b) W^T + b from T (M, C) bf16 and row-sum planes ([P][R][2] fp32, R = ln_rows or M when ln_rows == 0; rows
 * m >= R use the sums of row m - R: the shared classifier-free-guidance prefix), never normalising T: W / b (diffusers layout) are folded with
 * the LayerNorm gain / bias as the engine's loader folds them.  mode 0: GEGLU, W (2 inner, C) = [value rows | gate rows], b (2 inner) ->
 * out (M, inner) bf16.  mode 1: W (nseg C, C) = to_q [| to_k | to_v], nseg 1 | 3, heads * d == C, b (nseg C) or NULL, M = B * ntok -> q, k
 * [B][heads][ntok_pad][dp], vt [B][heads][dpv][ntok_pad] in the attention kernels' layout (dp = padded head dim, dpv = dp rounded up to 32,
 * ntok_pad = ntok rounded up to 32, q pre-scaled by log2(e) / sqrt(d), vt row dp = 1 where dpv > dp); k, vt unused when nseg == 1.
 * splitk as above (GEGLU cannot split).  mode 1 with planes, ln_g and ln_b all NULL: the same scatter without a LayerNorm (the OPT / CLIP
 * engines' QKV GEMM), on a 64 x 64-blocked copy of W where the engines block the matrix (N * C >= 4 Mi, C >= 1024; splitk 0 then picks the
 * blocked split).  Replaces norm1 + attn1.to_q/k/v, norm2 + attn2.to_q, norm3 + ff.net.0 of diffusers'
 * BasicTransformerBlock inside gill_unet_forward (reference call site: gill/custom_sd.py:633-638).  Synchronises. */
int gill_op_ln_gemm(int mode, const void* T_bf16, const float* planes, int P, int ln_rows, const float* ln_g, const float* ln_b, const void* W_bf16,
                    const float* b, void* out_bf16, void* q_bf16, void* k_bf16, void* vt_bf16, int M, int C, int inner, int nseg, int heads, int d,
                    int ntok, int splitk, void* stream);

/* fp8 (OCP e4m3) 3x3 convolution on CDNA4's v_mfma_scale_f32_16x16x128_f8f6f4 — BASELINE.json configs[4]; no reference
 * counterpart (the reference runs SD in fp16, gill/models.py:550-551).  x (B,H,W,Cin) bf16 NHWC, w (Cout,Cin,3,3) fp32,
 * optional bias (Cout) fp32 and residual (B,H,W,Cout) bf16 -> y (B,H,W,Cout) bf16.  Operands are quantised inside
 * (activations x 8 per tensor, weights per output channel).  splitk 0 = heuristic. */
int gill_op_conv3x3_fp8(const void* x_bf16, const float* w_oihw, const float* bias, const void* resid_bf16, void* y_bf16,
                        int B, int H, int W, int Cin, int Cout, int splitk, void* stream);

/* The fp8 mode's launchers one by one on QUANTISED operands (no reference counterpart; for the operator tests): every entry launches the
 * launcher the UNet engine launches and synchronises.  e4m3 tensors are plain bytes.
 * gill_conv_fp8_kpad: bytes per weight row of the fp8 convolution for Cin input channels (9 Cin rounded up to whole 128-byte K steps); -1
 *   unless Cin is a positive multiple of 64.  Host only.
 * gill_op_quant_fp8: y8[i] = fp8(scale * x[i]), saturating at +-448, NaN kept; n % 8 == 0.
 * gill_op_conv_weight_quant_fp8: w (Cout,Cin,3,3) of dtype GILL_DTYPE_* -> w8 [Cout][Kpad] in the kernel's K order (64-channel half
 *   q = tap * Cin / 64 + chunk, zero padding behind), colscale[o] = max|w_o| / 448 / act_scale (1 / act_scale for an all-zero row).
 * gill_op_conv3x3_fp8_q: y (B,H,W,Cout) bf16 = colscale[n] * (x8 (*) w8) + bias[n] + rowvec[b][n] + resid; x8 (B,H,W,Cin) e4m3.  splitk == 1:
 *   one launch; gn_stats (optional, with stats_bin > 0 dividing Cout): the GroupNorm partials of the output,
 *   [(b * (H W / 64) + slab) * (Cout / stats_bin) + bin][2] = {sum, sum of squares} over 64-row slabs, summed BEFORE the bf16 rounding.
 *   splitk > 1: ws [splitk][M][Cout] fp32 from the caller receives every slice's partial (accumulator times colscale; slices beyond the K
 *   steps hold zeros); then, unless partials_only, the split-K reducer adds them in slice order with bias, rowvec and residual.
 * gill_op_groupnorm_fp8: y8 (B,HW,C1+C2) = fp8(scale * [silu](GroupNorm(x1 ++ x2))), statistics from the tensors.
 * gill_op_linear_weight_quant_fp8: w (N,K) bf16 -> w8 [N][K], colscale[n] = max|w_n| / 448 / act_scale; K even.
 * gill_op_ln_quant_fp8: y8 (M,C) = fp8(act_scale * (t - mean) * rstd), mean / rstd of row m from stats [planes][R][2] fp32 {sum, sum of
 *   squares} added in plane order, R = ln_rows ? ln_rows : M; rows m >= ln_rows read row m - ln_rows.  C % 8 == 0.
 * gill_op_geglu_fp8_q: out (M, N/2) bf16 = (x8 . wv^T * sv + bv) * gelu(x8 . wg^T * sg + bg) with w8 [N][K], colscale, bias [N] in the
 *   PHYSICAL row order: rows 32 j .. 32 j + 15 are the value rows of outputs 16 j .. 16 j + 15, rows 32 j + 16 .. 32 j + 31 their gate rows.
 *   K % 128 == 0, N % 32 == 0. */
int gill_conv_fp8_kpad(int Cin);
int gill_op_quant_fp8(const void* x_bf16, float scale, int64_t n, void* y8, void* stream);
int gill_op_conv_weight_quant_fp8(const void* w_oihw, int dtype, int Cout, int Cin, float act_scale, void* w8, float* colscale, void* stream);
int gill_op_conv3x3_fp8_q(const void* x8, const void* w8, const float* colscale, const float* bias, const float* rowvec, const void* resid_bf16,
                          void* y_bf16, float* gn_stats, int stats_bin, float* ws, int partials_only, int B, int H, int W, int Cin, int Cout,
                          int splitk, void* stream);
int gill_op_groupnorm_fp8(const void* x1, int C1, const void* x2, int C2, int B, int HW, int groups, const float* gamma, const float* beta,
                          float eps, int silu, float scale, void* y8, void* stream);
int gill_op_linear_weight_quant_fp8(const void* w_bf16, int N, int K, float act_scale, void* w8, float* colscale, void* stream);
int gill_op_ln_quant_fp8(const void* t_bf16, int M, int C, const float* stats, int planes, int ln_rows, float eps, float act_scale, void* y8,
                         void* stream);
int gill_op_geglu_fp8_q(const void* x8, const void* w8, const float* colscale, const float* bias, void* out_bf16, int M, int N, int K,
                        void* stream);

/* The denoise loop's own kernels under a teacher: gill_sd_denoise_ex's table, stage kernel, step kernel and device step counter, with the UNet
 * replaced by "read this call's model output".  latents0 (B,n) fp32 (any n), model_out (ncalls,Bx,n) fp32 with Bx = 2B (uncond rows, then cond
 * rows) when guidance > 1, else B; noise (ncalls,B,n) fp32 or NULL as for gill_sd_denoise_ex -> lat_out (ncalls,B,n): the latents after every
 * call, unet_in_out (ncalls,B,n): the scaled UNet input of every call.  ncalls = gill_sd_schedule(...).  Synchronises. */
int gill_op_sd_sampler_run(const gill_sd_sampler* sampler, int v_prediction, int num_steps, float guidance, const float* latents0,
                           const float* model_out, const float* noise, int B, int64_t n, float* lat_out, float* unet_in_out, void* stream);
/* The same from step `start` (gill_sd_schedule_from's table): the first kernel is x = a * latents0 + b * init_noise, as in gill_sd_denoise_from. */
int gill_op_sd_sampler_run_from(const gill_sd_sampler* sampler, int v_prediction, int num_steps, int start, float guidance,
                                const float* latents0, const float* init_noise, const float* model_out, const float* noise, int B, int64_t n,
                                float* lat_out, float* unet_in_out, void* stream);
/* gill_sd_inpaint's kernels under the same teacher: the schedule, the stage / step / blend kernels, the keep table and the device step counter as
 * the loop drives them.  latent_mask (B,hw) fp32, hw dividing n (n = C * hw); masked_latents NULL: blend mode, n_in = n; masked_latents (B,n): concat
 * mode, n_in = (2 C + 1) * hw.  -> lat_out (ncalls,B,n) and unet_in_out (ncalls,Bx,n_in): BOTH CFG halves of every call's UNet input (Bx as for
 * model_out).  Synchronises. */
int gill_op_sd_inpaint_run(const gill_sd_sampler* sampler, int v_prediction, int num_steps, int start, float guidance, const float* latents0,
                           const float* init_noise, const float* latent_mask, const float* masked_latents, const float* model_out,
                           const float* noise, int B, int64_t n, int64_t hw, float* lat_out, float* unet_in_out, void* stream);

/* The kernels at the ends of the engines, each launched the way its engine launches it.  All synchronise.  For the operator tests.
 * conv_out (the UNet's predicted noise, the VAE's image and moments): x (B,H,W,Cin) bf16 NHWC, w (Cout,Cin,3,3) of w_dtype (GILL_DTYPE_*), optional
 * bias (Cout) fp32 -> y (B,Cout,H,W) fp32, 3x3 / pad 1.  The weights are re-laid as the loaders do; *path = the kernel that ran: 0 one wave per
 * pixel, 1 the matrix-pipe kernel with a run-time K loop, 2 | 4 | 10 the same with Cin / 32 fixed at compile time.  force_general: always path 0. */
int gill_op_conv_out(const void* x_bf16, const void* w_oihw, int w_dtype, const float* bias, float* y_f32, int B, int H, int W, int Cin, int Cout,
                     int force_general, int* path, void* stream);
/* conv_in of the UNet and the VAE: x (B,Cin,H,W) fp32 NCHW, w (Cout,Cin,3,3) of w_dtype, optional bias -> y (B,H,W,Cout) bf16 NHWC, as im2col
 * (pixels rounded to bf16, K = 9 Cin zero-padded to 64: 9 Cin <= 64, an error otherwise) + one GEMM.  counters (optional, ncounters 32-bit words):
 * cleared by the im2col launch, as the UNet forward clears its arrival counters. */
int gill_op_conv_in(const float* x_f32, const void* w_oihw, int w_dtype, const float* bias, void* y_bf16, int B, int Cin, int H, int W, int Cout,
                    uint32_t* counters, int ncounters, void* stream);
/* The same with K = 9 Cin zero-padded to a multiple of 64, as the engines' loaders do: 64 up to Cin = 7 (then gill_op_conv_in itself), 128 up to
 * Cin = 14 (the 9-channel inpainting UNet), an error beyond. */
int gill_op_conv_in_wide(const float* x_f32, const void* w_oihw, int w_dtype, const float* bias, void* y_bf16, int B, int Cin, int H, int W, int Cout,
                         uint32_t* counters, int ncounters, void* stream);
/* diffusers Timesteps(dim, flip_sin_to_cos = True, downscale_freq_shift = 0): t (n) fp32 -> out (n, dim) bf16 = [cos(t f_i) | sin(t f_i)],
 * f_i = 10000^(-i / (dim / 2)); dim even (an error otherwise). */
int gill_op_timestep_embed(const float* t, int n, int dim, void* out_bf16, void* stream);
/* The pre-LN transformer block's split-K reducer (csrc/tfm.hip): h (M,D) fp32 += sum of the sk slices of ws (sk,M,D) fp32 in slice order + bias,
 * in place; nb (M,D) bf16 = LayerNorm(h; g, b, eps).  D a multiple of 4, at most 8192 (an error otherwise). */
int gill_op_reduce_ln(const float* ws, int sk, int M, int D, const float* bias, float* h, const float* g, const float* b, void* nb_bf16, float eps,
                      void* stream);
/* h (M,N) fp32 += A (M,K) bf16 . W (N,K)^T + bias in place and nb (M,N) bf16 = LayerNorm(h; g, b, 1e-5), split `splitk` > 1 ways, the two ways
 * the block runs it: fuse = 1 partials + the reducer above, fuse = 0 the GEMM's own reducer + the stand-alone LayerNorm. */
int gill_op_linear_reduce_ln(const void* A_bf16, const void* W_bf16, const float* bias, float* h, const float* g, const float* b, void* nb_bf16,
                             int M, int N, int K, int splitk, int fuse, void* stream);
/* The tied lm_head: out (M,N) fp32 = x (M,K) bf16 . W (N,K)^T, 1 <= M <= 8, K a multiple of 8 (an error otherwise). */
int gill_op_skinny_gemm(const void* x_bf16, const void* W_bf16, float* out_f32, int M, int N, int K, void* stream);

/* ------------------------------------------------------------------------------------------
 * LM-head loss (csrc/lmloss.hip).  What HF's CrossEntropyLoss over lm_head(hidden_states[-1]) and utils.accuracy's topk
 * (gill/models.py:273-275, :363-365; gill/validate.py:89) read off a (B, T, vocab) logits tensor, without that tensor: the
 * rows are multiplied by the head on the matrix cores and only three numbers per row leave the kernel.
 *
 * X (M,D) bf16, W (V,D) bf16 row-major (the head as it lies in memory), target (M) int64 on the device: -100 = ignore, any
 * other value outside [0, V) is clamped (it lives on the device; the caller checks what it can see).  D % 32 == 0.  Per row:
 *   lse  = log sum_c exp(logit[c])                      (fp32 on the fp32-accumulated logits)
 *   tgt  = logit[target]
 *   rank = #{c != target : logit[c] > tgt or (logit[c] == tgt and c < target)}      (0 = top-1; rank < 5 = top-5)
 * and the row's loss is lse - tgt.  An ignored row gets rank -1 and lse = tgt = 0.  summary (nullable, 4 floats on the device)
 * = {mean loss over valid rows (NaN when none), n_valid, #rank < 1, #rank < 5}.  Five launches on `stream`, no host wait, no
 * float atomics, fixed summation orders: two calls give equal bits, and a row's results do not depend on the other rows.
 * Honours GILL_OP_REPEAT. */
int gill_op_lm_head_loss(const void* X_bf16, const void* W_bf16, const int64_t* target, int M, int V, int D, float* lse, float* tgt,
                         int32_t* rank, float* summary, void* stream);
/* How gill_op_lm_head_loss splits the work (host only, for tests): row tiles of *row_tile valid rows, MFMA column tiles of
 * *col_tile columns, *n_slabs vocabulary slabs of *cols_per_slab columns (the last one ragged) whose per-row partials a second
 * launch merges in ascending order.  The slabs cover [0, V) exactly once.  Any output may be NULL. */
int gill_lm_loss_geometry(int M, int V, int D, int* row_tile, int* col_tile, int* n_slabs, int* cols_per_slab);

/* ------------------------------------------------------------------------------------------
 * Image-block heads (csrc/img_heads.hip).  What generate_for_images_and_texts computes from the first [IMG] hidden state of a block
 * (gill/models.py:671-676 retrieval embedding, :698-704 decision MLP), for n blocks in one launch.
 *
 * hidden (rows, D) fp32, row_idx (n) int32 on the device: the flat row of each block's first [IMG] hidden state, in any order, repeats
 * allowed; a value outside [0, rows) is clamped on the device and nothing outside the buffers is touched.  Wr (E, D) bf16 with br (E)
 * fp32 and Wd (C, D) bf16 with bd (C) fp32 are nullable as pairs, not both.  D a multiple of 8, at most 8192; 1 <= E <= 1024;
 * 1 <= C <= 4; hidden and the weights 16-byte aligned.  Per block, with x = bf16(hidden[row]):
 *   ret_emb (n, E) fp32 = y / ||y||_2,  y = Wr x + br in fp32 (an all-zero y stays zero)
 *   probs (n, C) fp32 = softmax(z),  z = Wd x + bd;  choice (n) int32 = argmax z, a tie to the lower index
 * Outputs of an absent pair may be NULL.  One launch on `stream`, no host wait; an argument error is reported before anything is
 * enqueued.  No atomics and one fixed summation order: a block's outputs have the same bits at any n, at any position of row_idx and
 * on any run (the rule gill_attention_decode states for rows).  Honours GILL_OP_REPEAT. */
int gill_op_img_block_heads(const float* hidden_f32, int64_t rows, int D, const int32_t* row_idx, int n, const void* Wr_bf16, const float* br,
                            int E, const void* Wd_bf16, const float* bd, int C, float* ret_emb, float* probs, int32_t* choice, void* stream);
/* The CLIP rerank score (gill/models.py:733-751) of n blocks with g generated images each: visual (n g, E) fp32 un-normalised rows,
 * ret_emb (n, E) fp32 -> scores (n, g) fp32 = cos(visual[b g + j], ret_emb[b]), 0 where either row is all zero.  One launch, no host
 * wait; a score is a function of its own two rows alone (same bits at any n). */
int gill_op_img_rerank_scores(const float* visual_f32, const float* ret_emb_f32, int n, int g, int E, float* scores, void* stream);

/* What the GEMM / convolution launcher decides for a launch (host only, for tests; no GPU is touched).  Every decision of a launch — kernel
 * instantiation, grid, tile -> workgroup map, in-kernel finish, reducer — is made once, by a pure function of the arguments and of an environment
 * (pp = GILL_GEMM_PP, coop = GILL_GEMM_COOP, cus = compute units of the device), given explicitly here.
 * cases: n descriptors of GILL_GEMM_PLAN_CASE_INTS int32, in this order (pointers as 0 / 1 = absent / present):
 *   M N K lda ldc ldr K1 conv IH IW OH OW Cin stride ups pad_shift KX KX1 k_chunked alpha_is_one rows_per_batch resid_f32 act out_mode
 *   heads dp ntok splitk w_blk64 partials_only gn_groups gn_cg ln_planes wb_rows fn_cg
 *   A A2 X1 X2 W bias rowvec resid C ws gn_stats row_stats ln_stats ln_colsum fn_Y fn_gamma fn_beta coop_ctr fn_ss
 * rows: n rows of GILL_GEMM_PLAN_ROW_INTS int32:
 *   rc (0, or the error the launch would return: the rest of the row is then 0)
 *   k_nwv k_bn k_conv k_epi k_stages k_kt k_mi        the gemm_kernel template arguments
 *   grid_x grid_y grid_z
 *   ksteps ksteps_per_split tiles_m tiles_n npw groups_n nwv mi kt n_major xb_m xb_n M rows_per_batch     the kernel argument block's integers
 *   tile_rows ncls splitk coop reduce reduce_M        rows per M tile, parity classes, effective split, finish in-kernel, reducer launch follows (over reduce_M rows)
 *   row_planes gn_slab_rows coop_counters             what the engines ask before the launch */
#define GILL_GEMM_PLAN_CASE_INTS 54
#define GILL_GEMM_PLAN_ROW_INTS 34
int gill_gemm_plan(const int32_t* cases, int n, int pp, int coop, int cus, int32_t* rows);
/* What the launcher actually ran (host only, for tests): every successful GEMM / convolution launch of the calling thread copies its plan into a
 * ring of the 32 most recent ones.  Writes the most recent min(cap, 32, launches) plans into rows, oldest first, as rows of
 * GILL_GEMM_PLAN_ROW_INTS int32 in the layout above (rc = 0), sets *launched to the number of launches since the previous call and clears the
 * record.  cap == 0 (rows may be NULL) only counts and clears. */
int gill_gemm_plan_log(int32_t* rows, int cap, int* launched);
/* The engines' pre-launch choices under the same explicit environment (host only).  queries: n rows of 7 int32 = {what, six arguments}:
 *   0 split factor (M, N, K, act, plain, generic)    1 split factor on 64 x 64-blocked weights (M, N, K)    2 fused GroupNorm bins possible (N, cg)
 *   3 convolution on the ping-pong tile (rows, Cout)  4 chunk-major K order (HW, Cin, Cout)                  5 weights stored 64 x 64-blocked (N, K) */
int gill_gemm_query(const int32_t* queries, int n, int pp, int coop, int cus, int32_t* answers);

/* Which kernels a UNet transformer block (Transformer2DModel with one BasicTransformerBlock) runs (host only, for tests; no GPU is touched).  The
 * engine decides it in two pure steps: the weight layouts a layer is loaded with ("forms"), then what one call launches ("plan").  lnproj / xalg /
 * ffn_fused: the switches GILL_UNET_LNPROJ, GILL_UNET_XALG, GILL_UNET_FFN_FUSED (0 = off), given explicitly here.
 * cases: n descriptors of GILL_UNET_XF_PLAN_CASE_INTS int32:
 *   C heads ctx_len ctx_dim hw fp8 Bx shared      channels and heads of the layer, context tokens and width, tokens per sample at its level,
 *                                                 gill_unet_config.fp8_convs == 1, samples of the call, 1 = the shared prefix of a CFG pair (Bx counts the pair)
 * rows: n rows of GILL_UNET_XF_PLAN_ROW_INTS int32:
 *   lnproj xalg ffn_fused ffn_pre geglu_fp8       forms: fused projection pairs, two-GEMM cross-attention, fused feed-forward (PRE: it also runs
 *                                                 attn2.to_out), GEGLU projection in fp8
 *   lnproj gn_table cross ffn M M1                plan: fused projection pairs run, the block's GroupNorm arrives as a scale | shift table,
 *                                                 cross-attention 0 attention kernel / 1 two GEMMs, feed-forward 0 GEMMs / 1 GEMMs with the fp8 GEGLU /
 *                                                 2 fused / 3 fused PRE, rows of the call, rows up to the end of the self-attention */
#define GILL_UNET_XF_PLAN_CASE_INTS 8
#define GILL_UNET_XF_PLAN_ROW_INTS 11
int gill_unet_xf_plan(const int32_t* cases, int n, int lnproj, int xalg, int ffn_fused, int32_t* rows);

/* Which attention kernel gill_op_attention runs for a shape (host only, for tests; no GPU is touched).  The launcher decides it in one pure
 * function of the launch geometry — gill_op_attention's: head dim padded to 48 / 64 / 80 / 128 / 160, nq and nkv padded to multiples of 32 —
 * and of att_dma, the switch GILL_ATT_DMA (0 = off), given explicitly here.
 * out: GILL_ATTENTION_PLAN_INTS int32:
 *   family dp nthr grid        0 register-staged attention_kernel<dp, nthr> / 1 LDS-DMA attention_dma_kernel<dp, nthr>; padded head dim;
 *                              threads per workgroup (256 | 512 = 128 | 256 queries); workgroups launched */
#define GILL_ATTENTION_PLAN_INTS 4
int gill_attention_plan(int B, int H, int nq, int nkv, int d, int causal, int att_dma, int32_t* out);

/* Scoring pass of the OPT engine: gill_opt_img_hidden_ex (same embedding, same negative ids, same gathered rows; raw_out / emb_out
 * bit-equal to its outputs, either may be NULL) with the final LayerNorm on EVERY row, and row (b, t) scored against
 * labels[b][t + 1] by the fused loss above (HF's shifted CrossEntropyLoss).  labels (B,T) int64 on the device, -100 ignored; NULL
 * scores nothing (summary[0] is then NaN).
 *   token_loss (B, T-1) fp32, token_rank (B, T-1) int32: lse - tgt and the rank of every predicting position (0 / -1 where ignored)
 *   summary [4] fp32: {mean loss over the valid tokens of the whole batch, n_valid, #rank < 1, #rank < 5}
 *   last_logit_out (B, vocab) fp32, nullable: the logits row last_idx[b] - 1 (gill/models.py:419), through the GEMV of
 *     gill_opt_last_logits: bit-equal to that call fed the row of hidden_out
 *   hidden_out (B,T,D) fp32, nullable: hidden_states[-1]
 * last_idx_host may be NULL when raw_out, emb_out and last_logit_out are. */
int gill_opt_forward_loss(gill_opt* h, const int64_t* ids, const int32_t* last_idx_host, int B, int T, int num_tokens,
                          const void* extra_rows_bf16, int n_extra, const int64_t* labels, void* raw_out_bf16, void* emb_out_bf16,
                          float* token_loss, int32_t* token_rank, float* summary, float* last_logit_out, float* hidden_out, void* stream);


#ifdef __cplusplus
}
#endif
#endif /* GILL_AMD_H */
