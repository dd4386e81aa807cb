// Shared pre-LayerNorm transformer block (tfm.h): layer weight loader and w8 quantiser, workspace, and the runner whose launches are the OPT
// (forward, cached forward and the ragged decode step, on bf16 weights or e4m3 bytes), CLIP vision, CLIP text and mapper layer loops.
#include "tfm.h"

// REDUCE + RESIDUAL + LAYERNORM.  The narrow GEMMs of a layer (out_proj, fc2: N = D) run split-K; their reducer is also the natural place
// for the LayerNorm that follows them (the next sub-block's pre-LN): one workgroup per row adds the row's fp32 partials in split order, the
// bias and the fp32 residual stream (the order of gemm_reduce.hip's reducer epilogue), stores the new stream row, and — the row being complete in its
// registers — normalises it (two-pass variance like layernorm_kernel) into the bf16 operand of the next GEMM.  Two launches per layer gone
// (the LayerNorm passes) and the stream row is not re-read.  Fixed summation order: bit-repeatable.  (tests/test_ends_gpu.py holds the stream row to
// the bits of that order, and to the bits of the unfused way on the same operands.)
template <int VPT>      // float4 vectors per thread: D <= 1024 * VPT
__global__ __launch_bounds__(256) void opt_reduce_ln_kernel(const float* __restrict__ ws, int sk, int M, int D, const float* __restrict__ bias,
                                                            float* __restrict__ h, const float* __restrict__ g, const float* __restrict__ b,
                                                            bf16_t* __restrict__ nb, float eps) {
  __shared__ float red[8];
  const int row = blockIdx.x, tid = threadIdx.x, nv = D >> 2;
  const size_t slice = (size_t)M * D;
  // every load of the row goes out before the first addition (slices four at a time, clamped addresses: no branch between a load and its use,
  // so the compiler does not fence them one by one): the kernel is one memory round trip deep, not sk + 2
  float4 v[VPT], bb[VPT], rr[VPT];
  float4 q[VPT][4];
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int idx = (tid + i * 256 < nv) ? tid + i * 256 : 0;
    const int c = idx * 4;
    const float* p = ws + (size_t)row * D + c;
#pragma unroll
    for (int z = 0; z < 4; ++z) q[i][z] = *reinterpret_cast<const float4*>(p + (size_t)(z < sk ? z : 0) * slice);
    bb[i] = *reinterpret_cast<const float4*>(bias + c);
    rr[i] = *reinterpret_cast<const float4*>(h + (size_t)row * D + c);
  }
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int c = (tid + i * 256) * 4;
    const bool ok = tid + i * 256 < nv;
    float4 a = q[i][0];
#pragma unroll
    for (int z = 1; z < 4; ++z)
      if (z < sk) { a.x += q[i][z].x; a.y += q[i][z].y; a.z += q[i][z].z; a.w += q[i][z].w; }
    for (int z = 4; z < sk; ++z) {      // (more than four slices: not the OPT shapes)
      const float4 e = *reinterpret_cast<const float4*>(ws + (size_t)row * D + (ok ? c : 0) + (size_t)z * slice);
      a.x += e.x; a.y += e.y; a.z += e.z; a.w += e.w;
    }
    a.x = a.x + bb[i].x + rr[i].x; a.y = a.y + bb[i].y + rr[i].y; a.z = a.z + bb[i].z + rr[i].z; a.w = a.w + bb[i].w + rr[i].w;
    if (ok) *reinterpret_cast<float4*>(h + (size_t)row * D + c) = a;
    v[i] = ok ? a : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  auto block_sum = [&](float x) -> float {      // fixed order: lanes (xor tree), then the four waves in index order
    x = wave_sum(x);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = x;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
  };
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  const float mean = block_sum(s) / (float)D;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    if (tid + i * 256 < nv) {
      const float dx = v[i].x - mean, dy = v[i].y - mean, dz = v[i].z - mean, dw = v[i].w - mean;
      ss += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
  }
  const float rstd = rsqrtf(block_sum(ss) / (float)D + eps);
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int c = (tid + i * 256) * 4;
    if (tid + i * 256 < nv) {
      const float4 gg = *reinterpret_cast<const float4*>(g + c);
      const float4 be = *reinterpret_cast<const float4*>(b + c);
      uint2 o;
      o.x = pack_bf2((v[i].x - mean) * rstd * gg.x + be.x, (v[i].y - mean) * rstd * gg.y + be.y);
      o.y = pack_bf2((v[i].z - mean) * rstd * gg.z + be.z, (v[i].w - mean) * rstd * gg.w + be.w);
      *reinterpret_cast<uint2*>(nb + (size_t)row * D + c) = o;
    }
  }
}
int opt_reduce_ln_launch(const float* ws, int sk, int M, int D, const float* bias, float* h, const float* g, const float* b, bf16_t* nb,
                         float eps, hipStream_t s) {
  GILL_REQUIRE(D % 4 == 0 && D <= 8192 && sk >= 1, "reduce + LayerNorm: D must be a multiple of 4, at most 8192");
  if (D <= 1024) hipLaunchKernelGGL((opt_reduce_ln_kernel<1>), dim3(M), dim3(256), 0, s, ws, sk, M, D, bias, h, g, b, nb, eps);
  else if (D <= 4096) hipLaunchKernelGGL((opt_reduce_ln_kernel<4>), dim3(M), dim3(256), 0, s, ws, sk, M, D, bias, h, g, b, nb, eps);
  else hipLaunchKernelGGL((opt_reduce_ln_kernel<8>), dim3(M), dim3(256), 0, s, ws, sk, M, D, bias, h, g, b, nb, eps);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

int tfm_load_layer(const WeightTable& wt, DevPool& pool, const std::string& prefix, const TfmNames& names, int D, int F, bool stream64,
                   TfmLayer* L, hipStream_t s) {
  auto load_w = [&](const std::string& name, int N, int K, int blk, bf16_t* dst) -> int {
    const gill_tensor* t;
    GILL_TRY(wt.get(name + "weight", (int64_t)N * K, &t));
    return blk ? convert_to_bf16_blk64_launch(t->data, t->dtype, N, K, dst, s) : convert_to_bf16_launch(t->data, t->dtype, (int64_t)N * K, dst, s);
  };
  // geometry, layout and the owned bf16 matrix of m; the bias with it unless the caller fills its own
  auto mat = [&](TfmMat* m, const char* name, int N, int K) -> int {
    m->N = N; m->K = K; m->blk = stream64 ? gemm_stream64_weights(N, K) : 0;
    GILL_TRY(pool.alloc(&m->w, (size_t)N * K, false));
    if (!name) return pool.alloc(&m->b, (size_t)N, false);
    GILL_TRY(load_w(prefix + name, N, K, m->blk, m->w));
    return load_f32(wt, pool, prefix + name + "bias", N, &m->b, s);
  };
  auto norm_w = [&](const char* name, float** g, float** b) -> int {
    GILL_TRY(load_f32(wt, pool, prefix + name + "weight", D, g, s));
    return load_f32(wt, pool, prefix + name + "bias", D, b, s);
  };
  GILL_TRY(mat(&L->qkv, nullptr, 3 * D, D));
  // q | k | v stacked into [3D][D], or one packed in_proj copied whole (blocked or row-major, a [D][D] third of the stacked matrix is a
  // contiguous range of whole 64-row blocks)
  const int parts = names.qkv[1] ? 3 : 1, rows = 3 * D / parts;
  for (int j = 0; j < parts; ++j) {
    const gill_tensor* t;
    GILL_TRY(load_w(prefix + names.qkv[j], rows, D, L->qkv.blk, L->qkv.w + (size_t)j * rows * D));
    GILL_TRY(wt.get(prefix + names.qkv[j] + "bias", rows, &t));
    GILL_TRY(convert_to_f32_launch(t->data, t->dtype, rows, L->qkv.b + (size_t)j * rows, s));
  }
  GILL_TRY(mat(&L->o, names.o, D, D));
  GILL_TRY(mat(&L->fc1, names.fc1, F, D));
  GILL_TRY(mat(&L->fc2, names.fc2, D, F));
  GILL_TRY(norm_w(names.ln1, &L->ln1g, &L->ln1b));
  return norm_w(names.ln2, &L->ln2g, &L->ln2b);
}

int tfm_quantize_layer_w8(DevPool& pool, TfmLayer* L, hipStream_t s) {
  for (TfmMat* m : {&L->qkv, &L->o, &L->fc1, &L->fc2}) {
    GILL_TRY(pool.alloc(&m->w8, (size_t)m->N * m->K, false));
    GILL_TRY(pool.alloc(&m->scale, (size_t)m->N, false));
    GILL_TRY(w8_quant_launch(m->w, m->blk, m->N, m->K, m->w8, m->scale, s));
    GILL_TRY(w8_dequant_launch(m->w8, m->scale, m->N, m->K, m->blk, m->w, s));
  }
  return 0;
}

int tfm_linear_w8_launch(const bf16_t* A, int M, const unsigned char* W8, const float* scale, const float* b, int N, int K, const float* resid,
                         int act, void* out, bool out_f32, int splitk, float* ws, size_t ws_floats, const float* ln_g, const float* ln_b,
                         bf16_t* ln_out, hipStream_t s) {
  W8Args a;
  a.A = A; a.M = M; a.N = N; a.K = K; a.W8 = W8; a.scale = scale; a.bias = b; a.resid = resid; a.act = act; a.out_f32 = out_f32 ? 1 : 0; a.C = out;
  a.splitk = splitk; a.ws = ws; a.ws_floats = ws_floats;
  if (ln_out) {
    GILL_REQUIRE(out_f32 && resid == (const float*)out && act == ACT_NONE && b && ln_g && ln_b && N % 4 == 0 && N <= 8192,
                 "linear w8 + LayerNorm: an in-place fp32 residual launch with a bias, N a multiple of 4, at most 8192");
    a.partials_only = 1;
    GILL_TRY(linear_w8_launch(a, s));
    return opt_reduce_ln_launch(ws, linear_w8_splitk(a), M, N, b, (float*)out, ln_g, ln_b, ln_out, 1e-5f, s);
  }
  return linear_w8_launch(a, s);
}

int Tfm::alloc(DevPool& pool, int max_batch, int max_tok, int D_, int F_, int H_, int dp_, int dpv_, size_t ws_cap_floats) {
  D = D_; F = F_; H = H_; dp = dp_; dpv = dpv_;
  const size_t R = (size_t)max_batch * max_tok;
  const size_t Tpad = round_up(max_tok, 32);
  GILL_TRY(pool.alloc(&nbuf, R * D));
  GILL_TRY(pool.alloc(&ff, R * F));
  // q doubles as the decode mode's [rows][3D] projection (rows <= 16): 48 D elements at the least
  const size_t qn = (size_t)max_batch * H * Tpad * dp, qdec = (size_t)3 * 16 * D;
  GILL_TRY(pool.alloc(&q, qn > qdec ? qn : qdec));
  GILL_TRY(pool.alloc(&k, (size_t)max_batch * H * Tpad * dp));
  GILL_TRY(pool.alloc(&vt, (size_t)max_batch * H * dpv * Tpad));
  GILL_TRY(pool.alloc(&o, R * D));
  // split-K partials: gemm_pick_splitk() splits at most 16 ways; a launch whose partials would not fit runs unsplit (splitk())
  splitk_ws_floats = (size_t)16 * R * (size_t)(F > 3 * D ? F : 3 * D);
  if (ws_cap_floats && splitk_ws_floats > ws_cap_floats) splitk_ws_floats = ws_cap_floats;
  return pool.alloc(&splitk_ws, splitk_ws_floats, false);
}

int TfmRun::splitk(int M, int N, int K, int act, int blk) const {
  const int sk = blk ? gemm_pick_splitk_blk64(M, N, K) : gemm_pick_splitk(M, N, K, act);
  return (size_t)sk * M * N > t.splitk_ws_floats ? 1 : sk;
}

int tfm_linear_launch(const bf16_t* A, int M, const bf16_t* W, int blk, const float* b, int N, int K, const float* resid, int act, void* out,
                      bool out_f32, int splitk, float* ws, bool fuse_ln, const float* ln_g, const float* ln_b, bf16_t* ln_out, hipStream_t s) {
  GemmArgs g;
  g.M = M; g.N = N; g.K = K; g.K1 = K; g.A = A; g.lda = K; g.W = W; g.bias = b;
  g.resid = resid; g.ldr = N; g.resid_f32 = 1;
  g.act = act; g.out_mode = out_f32 ? OUT_F32 : OUT_BF16; g.C = out; g.ldc = N;
  g.w_blk64 = blk;
  g.splitk = splitk;
  g.ws = ws;
  if (fuse_ln && ln_out && g.splitk > 1 && out_f32 && resid == (const float*)out && act == ACT_NONE && b && N % 4 == 0 && N <= 8192) {
    g.partials_only = 1;
    GILL_TRY(gemm_launch(g, s));
    return opt_reduce_ln_launch(ws, g.splitk, M, N, b, (float*)out, ln_g, ln_b, ln_out, 1e-5f, s);
  }
  GILL_TRY(gemm_launch(g, s));
  if (ln_out) GILL_TRY(layernorm_launch(out, 1, ln_g, ln_b, ln_out, M, N, 1e-5f, s));
  return 0;
}

int TfmRun::linear(const bf16_t* A, int M, const TfmMat& m, const float* resid, int act, void* out, bool out_f32, const float* ln_g,
                   const float* ln_b, bf16_t* ln_out) const {
  // the e4m3 bytes (linear_w8.hip): the wide matrices (no residual) finish in the kernel, the narrow in-place ones split by the launcher's rule
  if (use_w8 && m.w8)
    return tfm_linear_w8_launch(A, M, m.w8, m.scale, m.b, m.N, m.K, resid, act, out, out_f32, resid ? 0 : 1, t.splitk_ws, t.splitk_ws_floats, ln_g,
                                ln_b, ln_out, s);
  return tfm_linear_launch(A, M, m.w, m.blk, m.b, m.N, m.K, resid, act, out, out_f32, splitk(M, m.N, m.K, act, m.blk), t.splitk_ws, t.fuse_ln, ln_g,
                           ln_b, ln_out, s);
}

int TfmRun::qkv(const bf16_t* A, int B, int ntok, const TfmMat& m, int nseg, int seg_base, int npad_q, int npad_kv, bf16_t* K, bf16_t* Vt,
                int kv_tok_offset) const {
  GemmArgs g;
  g.M = B * ntok; g.N = nseg * t.D; g.K = t.D; g.K1 = t.D; g.A = A; g.lda = t.D;
  g.W = m.w + (size_t)seg_base * t.D * t.D; g.bias = m.b + (size_t)seg_base * t.D;
  g.out_mode = OUT_QKV; g.Cq = t.q; g.Ck = K; g.Cvt = Vt;
  g.heads = t.H; g.dp = t.dp; g.dpv = t.dpv; g.ntok = ntok; g.ntok_pad_q = npad_q; g.ntok_pad_kv = npad_kv;
  g.seg_base = seg_base; g.kv_tok_offset = kv_tok_offset;
  g.qscale = 1.4426950408889634f / sqrtf((float)t.dp);   // log2(e) / sqrt(head dim): HF scales q by head_dim^-0.5, attention.hip works in log2
  g.w_blk64 = m.blk;
  g.splitk = t.split_qkv ? splitk(g.M, g.N, g.K, 0, m.blk) : 1;
  g.ws = t.splitk_ws;
  return gemm_launch(g, s);
}

int TfmRun::attend(int B, int nq, int nkv, int npad_q, int npad_kv, const bf16_t* K, const bf16_t* Vt, bool causal) const {
  AttnArgs a;
  a.Q = t.q; a.K = K; a.Vt = Vt; a.O = t.o;
  a.B = B; a.H = t.H; a.nq = nq; a.nkv = nkv; a.nq_pad = npad_q; a.nkv_pad = npad_kv;
  a.dp = t.dp; a.dpv = t.dpv; a.ldo = t.D; a.scale = 1.0f / sqrtf((float)t.dp); a.causal = causal;
  return attention_launch(a, s);
}

int TfmRun::self_attn(float* h, int B, int T, const TfmLayer& L, bool causal, const float* next_g, const float* next_b, const TfmKv* kv,
                      int past, const TfmDecode* dec) const {
  if (dec && dec->cu_new) {
    GILL_REQUIRE(kv && B == 1 && T >= 1 && dec->qkv, "extend attention: a cache and packed rows");
    GILL_TRY(linear(t.nbuf, T, L.qkv, nullptr, ACT_NONE, dec->qkv, false));
    if (dec->fork_parent) {
      GILL_REQUIRE(kv->fmt == GILL_KV_BF16 && dec->fork_plen, "fork attention: a bf16 cache, parents and prefix lengths");
      AttnForkArgs a;
      a.q = dec->qkv; a.k = dec->qkv + t.D; a.v = dec->qkv + 2 * t.D; a.ld = 3 * t.D;
      a.K = kv->k; a.Vt = kv->vt; a.parent = dec->fork_parent; a.plen = dec->fork_plen; a.cu_new = dec->cu_new; a.O = t.o; a.ldo = t.D;
      a.flags = dec->flags; a.C = dec->nseq; a.Bc = dec->fork_rows; a.total_new = T; a.max_new = dec->max_new; a.H = t.H; a.dp = t.dp;
      a.dpv = t.dpv; a.pitch = kv->pad; a.qscale = 1.4426950408889634f / sqrtf((float)t.dp);
      a.ws = dec->fork_ws; a.ws_bytes = dec->fork_ws_bytes;
      GILL_TRY(attention_fork_launch(a, s));
    } else if (kv->fmt == GILL_KV_E4M3) {
      AttnExtendKv8Args a;
      a.q = dec->qkv; a.k = dec->qkv + t.D; a.v = dec->qkv + 2 * t.D; a.ld = 3 * t.D;
      a.K8 = kv->k8; a.Vt8 = kv->vt8; a.Kexp = kv->kexp; a.Vexp = kv->vexp;
      a.lens = dec->lens; a.cu_new = dec->cu_new; a.O = t.o; a.ldo = t.D; a.flags = dec->flags;
      a.B = dec->nseq; a.total_new = T; a.max_new = dec->max_new; a.H = t.H; a.dp = t.dp; a.dpv = t.dpv; a.pitch = kv->pad;
      a.qscale = 1.4426950408889634f / sqrtf((float)t.dp);
      GILL_TRY(attention_extend_kv8_launch(a, s));
    } else {
      AttnExtendArgs a;
      a.q = dec->qkv; a.k = dec->qkv + t.D; a.v = dec->qkv + 2 * t.D; a.ld = 3 * t.D;
      a.K = kv->k; a.Vt = kv->vt; a.lens = dec->lens; a.cu_new = dec->cu_new; a.O = t.o; a.ldo = t.D; a.flags = dec->flags;
      a.B = dec->nseq; a.total_new = T; a.max_new = dec->max_new; a.H = t.H; a.dp = t.dp; a.dpv = t.dpv; a.pitch = kv->pad;
      a.qscale = 1.4426950408889634f / sqrtf((float)t.dp);
      GILL_TRY(attention_extend_launch(a, s));
    }
  } else if (dec && dec->br) {
    GILL_REQUIRE(kv && T == 1 && kv->fmt == GILL_KV_BF16 && dec->br_main && dec->br_gstart && dec->br_gparent && dec->br_gplen,
                 "branch attention: a bf16 cache, one token per branch and the groups");
    const TfmKv& bk = dec->br[kv - dec->br_main];
    GILL_TRY(linear(t.nbuf, B, L.qkv, nullptr, ACT_NONE, t.q, false));
    AttnBranchArgs a;
    a.q = t.q; a.k = t.q + t.D; a.v = t.q + 2 * t.D; a.ld = 3 * t.D;
    a.K = kv->k; a.Vt = kv->vt; a.Kb = bk.k; a.Vtb = bk.vt;
    a.gstart = dec->br_gstart; a.gparent = dec->br_gparent; a.gplen = dec->br_gplen; a.lens = dec->lens; a.O = t.o; a.ldo = t.D;
    a.flags = dec->flags; a.S = B; a.G = dec->br_groups; a.Sb = dec->br_rows; a.Bc = dec->br_main_rows; a.H = t.H; a.dp = t.dp; a.dpv = t.dpv;
    a.pitch = kv->pad; a.bpitch = bk.pad; a.qscale = 1.4426950408889634f / sqrtf((float)t.dp);
    GILL_TRY(attention_branch_launch(a, s));
  } else if (dec) {
    GILL_REQUIRE(kv && T >= 1, "decode attention: a cache");
    GILL_TRY(linear(t.nbuf, B * T, L.qkv, nullptr, ACT_NONE, t.q, false));
    if (kv->fmt == GILL_KV_E4M3) {
      GILL_REQUIRE(T == 1, "decode attention: an e4m3 KV cache takes one token per row (the multi-token append is not built for it)");
      AttnDecodeKv8Args a;
      a.q = t.q; a.k = t.q + t.D; a.v = t.q + 2 * t.D; a.ld = 3 * t.D;
      a.K8 = kv->k8; a.Vt8 = kv->vt8; a.Kexp = kv->kexp; a.Vexp = kv->vexp;
      a.lens = dec->lens; a.O = t.o; a.ldo = t.D; a.flags = dec->flags;
      a.B = B; a.H = t.H; a.dp = t.dp; a.dpv = t.dpv; a.pitch = kv->pad;
      a.qscale = 1.4426950408889634f / sqrtf((float)t.dp);
      GILL_TRY(attention_decode_kv8_launch(a, s));
    } else {
      AttnAppendArgs a;
      a.nq = T;
      a.q = t.q; a.k = t.q + t.D; a.v = t.q + 2 * t.D; a.ld = 3 * t.D;
      a.K = kv->k; a.Vt = kv->vt; a.lens = dec->lens; a.O = t.o; a.ldo = t.D; a.flags = dec->flags;
      a.B = B; a.H = t.H; a.dp = t.dp; a.dpv = t.dpv; a.pitch = kv->pad;
      a.qscale = 1.4426950408889634f / sqrtf((float)t.dp);
      GILL_TRY(T == 1 ? attention_decode_launch(a, s) : attention_append_launch(a, s));
    }
  } else {
    GILL_REQUIRE(!kv || kv->fmt != GILL_KV_E4M3, "flash attention: the cache is e4m3; this pass writes and reads a bf16 cache");
    const int Tpad = round_up(T, 32), kvpad = kv ? kv->pad : Tpad;
    bf16_t* kbuf = kv ? kv->k : t.k;
    bf16_t* vbuf = kv ? kv->vt : t.vt;
    GILL_TRY(qkv(t.nbuf, B, T, L.qkv, 3, 0, Tpad, kvpad, kbuf, vbuf, past));
    GILL_TRY(attend(B, T, past + T, Tpad, kvpad, kbuf, vbuf, causal));
  }
  return linear(t.o, B * T, L.o, h, ACT_NONE, h, true, next_g, next_b, next_g ? t.nbuf : nullptr);
}

int TfmRun::ffn(float* h, int rows, const TfmLayer& L, int act, const float* next_g, const float* next_b) const {
  GILL_TRY(linear(t.nbuf, rows, L.fc1, nullptr, act, t.ff, false));
  return linear(t.ff, rows, L.fc2, h, ACT_NONE, h, true, next_g, next_b, next_g ? t.nbuf : nullptr);
}

int TfmRun::layers(float* h, const TfmLayer* L, int n, int B, int T, int act, bool causal, const TfmKv* kv, int past, const TfmDecode* dec) const {
  if (n > 0) GILL_TRY(layernorm_launch(h, 1, L[0].ln1g, L[0].ln1b, t.nbuf, B * T, t.D, 1e-5f, s));
  for (int i = 0; i < n; ++i) {
    const TfmLayer* next = i + 1 < n ? &L[i + 1] : nullptr;
    GILL_TRY(self_attn(h, B, T, L[i], causal, L[i].ln2g, L[i].ln2b, kv ? &kv[i] : nullptr, past, dec));
    GILL_TRY(ffn(h, B * T, L[i], act, next ? next->ln1g : nullptr, next ? next->ln1b : nullptr));
  }
  return 0;
}
