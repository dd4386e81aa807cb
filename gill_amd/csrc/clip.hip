// CLIP vision tower (transformers CLIPVisionModel as the reference calls it: gill/models.py:78-96 builds it,
// :129-152 get_visual_embs reads `outputs.pooler_output`) on gfx950, through the same GEMM / attention / LayerNorm kernels
// as the OPT engine.
//   pixel_values (B,3,S,S) fp32 -> patch_embedding (PxP conv, stride P, no bias: im2col + MFMA GEMM) -> [class | patches]
//   + position_embedding -> pre_layrnorm -> L x { LN1, QKV (bias), softmax(QK^T/sqrt(d)) V, out_proj, +res, LN2, fc1,
//   quick_gelu, fc2, +res } -> post_layernorm(row 0) = pooler_output (B, D) fp32.
// fp32 residual stream, bf16 GEMM operands, fp32 accumulation (as opt.hip).  The L layers are the shared block of tfm.h.
#include "tfm.h"

struct gill_clip {
  gill_clip_config cfg;
  DevPool pool;
  int ntok = 0, npatch = 0, kpatch = 0, kpad = 0;
  TfmMat patch;               // [D][kpad], no bias: patch_embedding.weight flattened (c, ky, kx), zero-padded to a multiple of 64
  float* cls = nullptr;       // [D]
  float* pos = nullptr;       // [ntok][D]
  float *preg = nullptr, *preb = nullptr, *postg = nullptr, *postb = nullptr;
  std::vector<TfmLayer> layers;
  Tfm tfm;
  // workspace
  bf16_t* col = nullptr;      // [B*npatch][kpad]
  float* h = nullptr;         // [B*ntok][D]
  float* gath = nullptr;      // [B][D]
  int32_t* idx_dev = nullptr; // [B]
};

// col[(b*npatch + py*G + px)][(c*P + ky)*P + kx] = bf16(pixel[b][c][py*P + ky][px*P + kx]); columns >= 3*P*P are zero
__global__ __launch_bounds__(256) void clip_im2col_kernel(const float* __restrict__ px, int B, int S, int P, int G, int kpatch,
                                                          int kpad, bf16_t* __restrict__ col) {
  const int64_t total = (int64_t)B * G * G * kpad;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int kcol = (int)(i % kpad);
    const int64_t row = i / kpad;
    float v = 0.f;
    if (kcol < kpatch) {
      const int kx = kcol % P, ky = (kcol / P) % P, c = kcol / (P * P);
      const int pxi = (int)(row % G), pyi = (int)((row / G) % G), b = (int)(row / ((int64_t)G * G));
      v = px[(((int64_t)b * 3 + c) * S + pyi * P + ky) * S + pxi * P + kx];
    }
    col[i] = f2bf(v);
  }
}

// h[b][0][:] = class_embedding + pos[0]; h[b][1+p][:] += pos[1+p]   (rows 1.. were written by the patch GEMM)
__global__ __launch_bounds__(256) void clip_embed_finish_kernel(float* __restrict__ h, const float* __restrict__ cls,
                                                                const float* __restrict__ pos, int ntok, int D) {
  const int row = blockIdx.x;          // b * ntok + t
  const int t = row % ntok;
  float* o = h + (size_t)row * D;
  const float* pe = pos + (size_t)t * D;
  for (int c = threadIdx.x; c < D; c += blockDim.x) o[c] = (t == 0 ? cls[c] : o[c]) + pe[c];
}

extern "C" int gill_clip_create(gill_clip** out, const gill_clip_config* cfg, const gill_tensor* weights, int n_weights) {
  GILL_REQUIRE(out && cfg && weights, "null argument");
  const int D = cfg->hidden_size, F = cfg->intermediate_size, H = cfg->num_heads, P = cfg->patch_size, S = cfg->image_size;
  GILL_REQUIRE(D % 64 == 0 && F % 64 == 0 && H > 0 && D % H == 0, "CLIP dims must be multiples of 64");
  GILL_REQUIRE(P > 0 && S % P == 0 && cfg->max_batch >= 1 && cfg->num_layers >= 1, "bad CLIP geometry");
  const int hd = D / H;
  GILL_REQUIRE(attn_padded_dim(hd) == hd, "CLIP head dim must be one of 48/64/80/128/160");
  gill_clip* m = new gill_clip();
  m->cfg = *cfg;
  const int G = S / P;
  m->npatch = G * G; m->ntok = m->npatch + 1; m->kpatch = 3 * P * P; m->kpad = round_up(m->kpatch, 64);
  WeightTable wt(weights, n_weights);
  hipStream_t s = nullptr;
  int rc = 0;
  auto fail = [&](int r) { delete m; return r; };
  const std::string vm = "vision_model.";
  {
    // patch_embedding.weight [D][3][P][P] -> bf16 [D][kpad] (zero padded columns)
    const gill_tensor* t;
    if ((rc = wt.get(vm + "embeddings.patch_embedding.weight", (int64_t)D * m->kpatch, &t))) return fail(rc);
    bf16_t* tmp;
    if ((rc = m->pool.alloc(&tmp, (size_t)D * m->kpatch, false))) return fail(rc);
    if ((rc = convert_to_bf16_launch(t->data, t->dtype, (int64_t)D * m->kpatch, tmp, s))) return fail(rc);
    m->patch.N = D; m->patch.K = m->kpad;
    if ((rc = m->pool.alloc(&m->patch.w, (size_t)D * m->kpad, true))) return fail(rc);
    if (hipMemcpy2D(m->patch.w, sizeof(bf16_t) * m->kpad, tmp, sizeof(bf16_t) * m->kpatch, sizeof(bf16_t) * m->kpatch, D,
                    hipMemcpyDeviceToDevice) != hipSuccess) { gill_set_error("clip create: weight re-layout failed"); return fail(-1); }
  }
  if ((rc = load_f32(wt, m->pool, vm + "embeddings.class_embedding", D, &m->cls, s))) return fail(rc);
  if ((rc = load_f32(wt, m->pool, vm + "embeddings.position_embedding.weight", (int64_t)m->ntok * D, &m->pos, s))) return fail(rc);
  if ((rc = load_f32(wt, m->pool, vm + "pre_layrnorm.weight", D, &m->preg, s))) return fail(rc);   // (sic: the HF name)
  if ((rc = load_f32(wt, m->pool, vm + "pre_layrnorm.bias", D, &m->preb, s))) return fail(rc);
  if ((rc = load_f32(wt, m->pool, vm + "post_layernorm.weight", D, &m->postg, s))) return fail(rc);
  if ((rc = load_f32(wt, m->pool, vm + "post_layernorm.bias", D, &m->postb, s))) return fail(rc);
  m->layers.resize(cfg->num_layers);
  const TfmNames names = {{"self_attn.q_proj.", "self_attn.k_proj.", "self_attn.v_proj."}, "self_attn.out_proj.", "mlp.fc1.", "mlp.fc2.",
                          "layer_norm1.", "layer_norm2."};
  // row-major weights, not the STREAM64 layout: kept as found
  for (int i = 0; i < cfg->num_layers; ++i)
    if ((rc = tfm_load_layer(wt, m->pool, vm + "encoder.layers." + std::to_string(i) + ".", names, D, F, false, &m->layers[i], s)))
      return fail(rc);
  if ((rc = m->pool.alloc(&m->col, (size_t)cfg->max_batch * m->npatch * m->kpad))) return fail(rc);
  if ((rc = m->pool.alloc(&m->h, (size_t)cfg->max_batch * m->ntok * D))) return fail(rc);
  // fuse_ln stays off (every LayerNorm a launch of its own) and the split-K workspace uncapped: kept as found
  if ((rc = m->tfm.alloc(m->pool, cfg->max_batch, m->ntok, D, F, H, hd, round_up(hd, 32)))) return fail(rc);
  if ((rc = m->pool.alloc(&m->gath, (size_t)cfg->max_batch * D))) return fail(rc);
  if ((rc = m->pool.alloc(&m->idx_dev, (size_t)cfg->max_batch))) return fail(rc);
  {
    std::vector<int32_t> idx(cfg->max_batch);
    for (int b = 0; b < cfg->max_batch; ++b) idx[b] = b * m->ntok;     // the class-token row of every image
    if (hipMemcpy(m->idx_dev, idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice) != hipSuccess) {
      gill_set_error("clip create: index upload failed"); return fail(-1);
    }
  }
  if (hipDeviceSynchronize() != hipSuccess) { gill_set_error("clip create: device sync failed"); return fail(-1); }
  *out = m;
  return 0;
}

extern "C" void gill_clip_destroy(gill_clip* h) { delete h; }

extern "C" int gill_clip_forward(gill_clip* m, const float* pixel_values, int B, float* pooled_out, void* stream) {
  GILL_REQUIRE(m && pixel_values && pooled_out, "null argument");
  GILL_REQUIRE(B >= 1 && B <= m->cfg.max_batch, "batch exceeds the CLIP handle's max_batch");
  hipStream_t s = (hipStream_t)stream;
  const gill_clip_config& c = m->cfg;
  const int D = c.hidden_size, T = m->ntok, R = B * T;
  const TfmRun r{m->tfm, s};
  {
    const int64_t total = (int64_t)B * m->npatch * m->kpad;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 32768) blocks = 32768;
    hipLaunchKernelGGL(clip_im2col_kernel, dim3(blocks), dim3(256), 0, s, pixel_values, B, c.image_size, c.patch_size,
                       c.image_size / c.patch_size, m->kpatch, m->kpad, m->col);
    GILL_CHECK_HIP(hipGetLastError());
    for (int b = 0; b < B; ++b)      // rows b*T+1 .. of the fp32 stream (row b*T is the class token)
      GILL_TRY(r.linear(m->col + (size_t)b * m->npatch * m->kpad, m->npatch, m->patch, nullptr, ACT_NONE, m->h + ((size_t)b * T + 1) * D, true));
    hipLaunchKernelGGL(clip_embed_finish_kernel, dim3(R), dim3(256), 0, s, m->h, m->cls, m->pos, T, D);
    GILL_CHECK_HIP(hipGetLastError());
  }
  GILL_TRY(layernorm_f32out_launch(m->h, 1, m->preg, m->preb, m->h, R, D, 1e-5f, s));   // in place, row by row
  GILL_TRY(r.layers(m->h, m->layers.data(), (int)m->layers.size(), B, T, ACT_QUICK_GELU, false));
  // pooler_output = post_layernorm(last_hidden_state[:, 0])
  GILL_TRY(gather_rows_launch(m->h, 1, m->idx_dev, B, D, m->gath, 1, s));
  GILL_TRY(layernorm_f32out_launch(m->gath, 1, m->postg, m->postb, pooled_out, B, D, 1e-5f, s));
  return 0;
}
