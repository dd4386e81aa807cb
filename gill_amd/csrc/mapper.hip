// Stage 2 — GILLMapper: gill.layers.TextFcLayer(mode='gill_mapper').forward  (reference
// gill/layers.py:28-53; module built at layers.py:17-24).
//
//   x = x + input_embs                                    layers.py:31-32
//   x = fc(x)                         Linear(in_dim, 512)  layers.py:42
//   x = tfm(src=x, tgt=query_embs)    nn.Transformer(d=512, nhead=4, enc 4 / dec 4, ff 2048, ReLU,
//                                     norm_first, eps 1e-5, no masks)          layers.py:43
//   out = model(x)                    Linear(512, out_dim) layers.py:44
//
// The residual stream is kept in fp32 (rows are few: 8 and 77 per sample); every GEMM runs bf16 x bf16
// on MFMA with fp32 accumulation; attention is the shared flash kernel (4 heads x 128).  The encoder layers and the
// self-attention and feed-forward parts of the decoder layers are the shared block of tfm.h.
#include "tfm.h"

namespace {

struct NormW { float* g = nullptr; float* b = nullptr; };
struct DecLayer { TfmLayer blk; TfmMat ca_in, ca_out; NormW ca_norm; };   // blk: self_attn (norm1) + feed-forward (norm3); ca: multihead_attn (norm2)

}  // namespace

struct gill_mapper {
  gill_mapper_config cfg;
  DevPool pool;
  TfmMat fc, model;
  float* query = nullptr;  // (n_out, hidden) fp32
  std::vector<TfmLayer> enc;
  std::vector<DecLayer> dec;
  NormW enc_norm, dec_norm;
  // workspace (sized for max_batch)
  bf16_t* x0 = nullptr;     // (B*8, in_dim)
  float* h_enc = nullptr;   // (B*8, hidden)
  float* h_dec = nullptr;   // (B*77, hidden)
  bf16_t* mem = nullptr;    // (B*8, hidden) encoder output
  Tfm tfm;                  // nbuf / ff / o serve the encoder (B*8 rows) and the decoder (B*77 rows)
};

static int load_linear(const WeightTable& wt, DevPool& pool, const std::string& wname, const std::string& bname, int out,
                       int in, TfmMat* l, hipStream_t s) {
  l->N = out; l->K = in;
  GILL_TRY(load_bf16(wt, pool, wname, (int64_t)out * in, &l->w, s));
  GILL_TRY(load_f32(wt, pool, bname, out, &l->b, s));
  return 0;
}
static int load_norm(const WeightTable& wt, DevPool& pool, const std::string& prefix, int dim, NormW* n, hipStream_t s) {
  GILL_TRY(load_f32(wt, pool, prefix + ".weight", dim, &n->g, s));
  GILL_TRY(load_f32(wt, pool, prefix + ".bias", dim, &n->b, s));
  return 0;
}

extern "C" int gill_mapper_create(gill_mapper** out, const gill_mapper_config* cfg, const gill_tensor* weights,
                                  int n_weights) {
  GILL_REQUIRE(out && cfg && weights, "null argument");
  GILL_REQUIRE(cfg->hidden_dim % 64 == 0 && cfg->in_dim % 64 == 0 && cfg->ffn_dim % 64 == 0,
               "mapper dims must be multiples of 64");
  GILL_REQUIRE(cfg->hidden_dim % cfg->num_heads == 0, "hidden_dim must divide by num_heads");
  const int hd = cfg->hidden_dim / cfg->num_heads;
  GILL_REQUIRE(attn_padded_dim(hd) == hd, "mapper head dim must be one of 48/64/80/128/160");
  GILL_REQUIRE(cfg->max_batch > 0, "max_batch must be positive");
  gill_mapper* m = new gill_mapper();
  m->cfg = *cfg;
  WeightTable wt(weights, n_weights);
  hipStream_t s = nullptr;
  const int Hd = cfg->hidden_dim, F = cfg->ffn_dim;
  int rc = 0;
  auto fail = [&](int r) { delete m; return r; };
  if ((rc = load_linear(wt, m->pool, "fc.weight", "fc.bias", Hd, cfg->in_dim, &m->fc, s))) return fail(rc);
  if ((rc = load_linear(wt, m->pool, "model.weight", "model.bias", cfg->out_dim, Hd, &m->model, s))) return fail(rc);
  if ((rc = load_f32(wt, m->pool, "query_embs", (int64_t)cfg->num_output_tokens * Hd, &m->query, s))) return fail(rc);
  // nn.Transformer packs q | k | v as in_proj; row-major weights, not the STREAM64 layout: kept as found
  const TfmNames enc_names = {{"self_attn.in_proj_", nullptr, nullptr}, "self_attn.out_proj.", "linear1.", "linear2.", "norm1.", "norm2."};
  const TfmNames dec_names = {{"self_attn.in_proj_", nullptr, nullptr}, "self_attn.out_proj.", "linear1.", "linear2.", "norm1.", "norm3."};
  m->enc.resize(cfg->num_enc_layers);
  for (int i = 0; i < cfg->num_enc_layers; ++i)
    if ((rc = tfm_load_layer(wt, m->pool, "tfm.encoder.layers." + std::to_string(i) + ".", enc_names, Hd, F, false, &m->enc[i], s)))
      return fail(rc);
  if ((rc = load_norm(wt, m->pool, "tfm.encoder.norm", Hd, &m->enc_norm, s))) return fail(rc);
  m->dec.resize(cfg->num_dec_layers);
  for (int i = 0; i < cfg->num_dec_layers; ++i) {
    const std::string p = "tfm.decoder.layers." + std::to_string(i) + ".";
    DecLayer& L = m->dec[i];
    if ((rc = tfm_load_layer(wt, m->pool, p, dec_names, Hd, F, false, &L.blk, s))) return fail(rc);
    if ((rc = load_linear(wt, m->pool, p + "multihead_attn.in_proj_weight", p + "multihead_attn.in_proj_bias", 3 * Hd, Hd, &L.ca_in, s)))
      return fail(rc);
    if ((rc = load_linear(wt, m->pool, p + "multihead_attn.out_proj.weight", p + "multihead_attn.out_proj.bias", Hd, Hd, &L.ca_out, s)))
      return fail(rc);
    if ((rc = load_norm(wt, m->pool, p + "norm2", Hd, &L.ca_norm, s))) return fail(rc);
  }
  if ((rc = load_norm(wt, m->pool, "tfm.decoder.norm", Hd, &m->dec_norm, s))) return fail(rc);

  const size_t B = cfg->max_batch;
  const size_t Ti = cfg->num_input_tokens, To = cfg->num_output_tokens;
  if ((rc = m->pool.alloc(&m->x0, B * Ti * cfg->in_dim))) return fail(rc);
  if ((rc = m->pool.alloc(&m->h_enc, B * Ti * Hd))) return fail(rc);
  if ((rc = m->pool.alloc(&m->h_dec, B * To * Hd))) return fail(rc);
  if ((rc = m->pool.alloc(&m->mem, B * Ti * Hd))) return fail(rc);
  if ((rc = m->tfm.alloc(m->pool, cfg->max_batch, (int)(To > Ti ? To : Ti), Hd, F, cfg->num_heads, hd, round_up(hd, 32)))) return fail(rc);
  // QKV GEMMs run unsplit, fuse_ln stays off (every LayerNorm a launch of its own): kept as found
  m->tfm.split_qkv = false;
  if (hipDeviceSynchronize() != hipSuccess) { gill_set_error("mapper create: device sync failed"); return fail(-1); }
  *out = m;
  return 0;
}

extern "C" void gill_mapper_destroy(gill_mapper* h) { delete h; }

extern "C" int gill_mapper_forward(gill_mapper* m, const void* x_bf16, const void* input_embs_bf16, int B, int Be,
                                   float* out, void* stream) {
  GILL_REQUIRE(m && x_bf16 && out, "null argument");
  GILL_REQUIRE(B >= 1 && B <= m->cfg.max_batch, "batch exceeds max_batch of the mapper handle");
  GILL_REQUIRE(input_embs_bf16 == nullptr || Be == 1 || Be == B, "input_embs batch must be 1 or B");
  hipStream_t s = (hipStream_t)stream;
  const TfmRun r{m->tfm, s};
  const Tfm& t = m->tfm;
  const gill_mapper_config& c = m->cfg;
  const int Ti = c.num_input_tokens, To = c.num_output_tokens, Hd = c.hidden_dim;
  // x = x + input_embs (layers.py:31-32); bf16 operand for the first MFMA GEMM
  const bf16_t* x0 = (const bf16_t*)x_bf16;
  if (input_embs_bf16) {
    const int64_t n = (int64_t)B * Ti * c.in_dim;
    const int64_t period = (Be == 1) ? (int64_t)Ti * c.in_dim : n;
    GILL_TRY(add_cast_launch(x_bf16, 0, input_embs_bf16, 0, n, period, m->x0, s));
    x0 = m->x0;
  }
  // fc (layers.py:42) -> fp32 encoder stream
  GILL_TRY(r.linear(x0, B * Ti, m->fc, nullptr, ACT_NONE, m->h_enc, true));
  GILL_TRY(r.layers(m->h_enc, m->enc.data(), (int)m->enc.size(), B, Ti, ACT_RELU, false));
  GILL_TRY(layernorm_launch(m->h_enc, 1, m->enc_norm.g, m->enc_norm.b, m->mem, B * Ti, Hd, 1e-5f, s));
  // tgt = query_embs.repeat(B,1,1) (layers.py:43)
  for (int b = 0; b < B; ++b)
    GILL_CHECK_HIP(hipMemcpyAsync(m->h_dec + (size_t)b * To * Hd, m->query, sizeof(float) * To * Hd,
                                  hipMemcpyDeviceToDevice, s));
  const int To_pad = round_up(To, 32), Ti_pad = round_up(Ti, 32);
  for (const DecLayer& L : m->dec) {
    GILL_TRY(layernorm_launch(m->h_dec, 1, L.blk.ln1g, L.blk.ln1b, t.nbuf, B * To, Hd, 1e-5f, s));
    GILL_TRY(r.self_attn(m->h_dec, B, To, L.blk, false, L.ca_norm.g, L.ca_norm.b));
    // cross attention: q from the target stream, k/v from the encoder memory
    GILL_TRY(r.qkv(t.nbuf, B, To, L.ca_in, 1, 0, To_pad, Ti_pad, t.k, t.vt, 0));
    GILL_TRY(r.qkv(m->mem, B, Ti, L.ca_in, 2, 1, To_pad, Ti_pad, t.k, t.vt, 0));
    GILL_TRY(r.attend(B, To, Ti, To_pad, Ti_pad, t.k, t.vt, false));
    GILL_TRY(r.linear(t.o, B * To, L.ca_out, m->h_dec, ACT_NONE, m->h_dec, true, L.blk.ln2g, L.blk.ln2b, t.nbuf));
    GILL_TRY(r.ffn(m->h_dec, B * To, L.blk, ACT_RELU));
  }
  GILL_TRY(layernorm_launch(m->h_dec, 1, m->dec_norm.g, m->dec_norm.b, t.nbuf, B * To, Hd, 1e-5f, s));
  // model (layers.py:44)
  return r.linear(t.nbuf, B * To, m->model, nullptr, ACT_NONE, out, true);
}
