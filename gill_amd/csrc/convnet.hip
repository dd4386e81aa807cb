// Load-time half of convnet.h: the weight forms the conv stacks of the UNet and the VAE decoder share.
#include "convnet.h"
#include <stdlib.h>

__global__ void vec_add_f32_kernel(const float* a, const float* b, int n, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}

bool conv_ups4_enabled() {
  static const int on = [] { const char* v = getenv("GILL_CONV_UPS4"); return v ? atoi(v) : 1; }();
  return on != 0;
}

int load_norm(const WeightTable& wt, DevPool& pool, hipStream_t s, const std::string& p, int c, NormW* n) {
  n->c = c;
  GILL_TRY(load_f32(wt, pool, p + ".weight", c, &n->g, s));
  return load_f32(wt, pool, p + ".bias", c, &n->b, s);
}

int load_conv3(const WeightTable& wt, DevPool& pool, hipStream_t s, const std::string& p, int cin, int cout, int hw, ConvW* c, bool f8,
               bool ups4) {
  c->cin = cin; c->cout = cout; c->chunked = conv_k_chunked(hw, cin, cout) ? 1 : 0;
  const gill_tensor* t;
  GILL_TRY(wt.get(p + ".weight", (int64_t)cout * cin * 9, &t));
  if (ups4 && conv_ups4_enabled() && !f8) {
    c->ups4 = 1; c->chunked = 0;
    GILL_TRY(pool.alloc(&c->w, (size_t)16 * cout * cin, false));
    GILL_TRY(conv_weight_relayout_ups4_launch(t->data, t->dtype, cout, cin, c->w, s));
  } else if (f8) {
    c->kpad = conv_fp8_kpad(cin);
    GILL_TRY(pool.alloc(&c->w8, (size_t)cout * c->kpad, false));
    GILL_TRY(pool.alloc(&c->cs, (size_t)cout, false));
    GILL_TRY(conv_weight_quant_fp8_launch(t->data, t->dtype, cout, cin, F8_ACT_SCALE, c->w8, c->cs, s));
  } else {
    GILL_TRY(pool.alloc(&c->w, (size_t)cout * cin * 9, false));
    if (c->chunked) GILL_TRY(conv_weight_relayout_chunked_launch(t->data, t->dtype, cout, cin, c->w, s));
    else GILL_TRY(conv_weight_relayout_launch(t->data, t->dtype, cout, cin, c->w, s));
  }
  return load_f32(wt, pool, p + ".bias", cout, &c->b, s);
}

int copy_rows_bf16(const bf16_t* src, int rows, int cols, bf16_t* dst, int dst_ld, hipStream_t s) {
  GILL_CHECK_HIP(hipMemcpy2DAsync(dst, sizeof(bf16_t) * dst_ld, src, sizeof(bf16_t) * cols, sizeof(bf16_t) * cols, rows,
                                  hipMemcpyDeviceToDevice, s));
  return 0;
}

int conv_in_im2col_weight(const void* w_oihw, int dtype, int cin, int cout, bf16_t* tmp, bf16_t* w64, hipStream_t s) {
  GILL_TRY(conv_weight_relayout_launch(w_oihw, dtype, cout, cin, tmp, s));
  return copy_rows_bf16(tmp, cout, cin * 9, w64, conv_in_kpad(cin), s);
}

int load_conv_in_im2col(const WeightTable& wt, DevPool& pool, hipStream_t s, const std::string& p, int cin, int cout, bf16_t** w, float** b) {
  const int kk = cin * 9;
  GILL_REQUIRE(cin >= 1 && cin <= CONV_IN_MAX_CIN, "conv_in: in_channels must be 1 .. 14 (9 * in_channels fits two 64-wide K steps)");
  const gill_tensor* t;
  bf16_t* tmp;
  GILL_TRY(wt.get(p + ".weight", (int64_t)cout * kk, &t));
  GILL_TRY(pool.alloc(&tmp, (size_t)cout * kk, false));
  GILL_TRY(pool.alloc(w, (size_t)cout * conv_in_kpad(cin), true));
  GILL_TRY(conv_in_im2col_weight(t->data, t->dtype, cin, cout, tmp, *w, s));
  return load_f32(wt, pool, p + ".bias", cout, b, s);
}

int load_conv_out(const WeightTable& wt, DevPool& pool, hipStream_t s, const std::string& p, int cin, int cout, bf16_t** w, float** b) {
  const gill_tensor* t;
  GILL_TRY(wt.get(p + ".weight", (int64_t)cout * cin * 9, &t));
  GILL_TRY(pool.alloc(w, (size_t)cout * cin * 9, false));
  GILL_TRY(conv_weight_relayout_launch(t->data, t->dtype, cout, cin, *w, s));
  return load_f32(wt, pool, p + ".bias", cout, b, s);
}

int fuse_shortcut_into_conv2(DevPool& pool, hipStream_t s, const bf16_t* sc_w, const float* sc_b, ResW* r) {
  const int cin = r->cin, cout = r->cout, kf = 9 * cout + cin;
  GILL_TRY(pool.alloc(&r->c2f_w, (size_t)cout * kf, false));
  GILL_TRY(copy_rows_bf16(r->c2.w, cout, 9 * cout, r->c2f_w, kf, s));
  GILL_TRY(copy_rows_bf16(sc_w, cout, cin, r->c2f_w + 9 * cout, kf, s));
  GILL_TRY(pool.alloc(&r->c2f_b, (size_t)cout, false));
  hipLaunchKernelGGL(vec_add_f32_kernel, dim3(cdiv(cout, 256)), dim3(256), 0, s, r->c2.b, sc_b, cout, r->c2f_b);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}
