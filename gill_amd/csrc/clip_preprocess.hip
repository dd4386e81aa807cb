// CLIP image preprocessing on the device (gill/utils.py:111-119, the feature extractor called at gill/models.py:606-613): resize of the shortest
// edge to `size` with Pillow's BICUBIC resampler, centre crop to size x size, scale to [0, 1], normalise with the CLIP mean / std.
//
// Pillow's 8-bit resampler is integer arithmetic, reproduced here bit for bit:
//   per axis  scale = in / out, fs = max(scale, 1), support = 2 fs; per output index xx: center = (xx + 0.5) scale, the window
//             [xmin, xmax) = [max(int(center - support + 0.5), 0), min(int(center + support + 0.5), in)), weights cubic((x + xmin - center + 0.5) / fs)
//             (a = -0.5) divided by their sum, all in doubles, then k = (int)(w 2^22 +- 0.5) truncated toward zero;
//   a pass    out = clip((2^21 + sum k[x] px[xmin + x]) >> 22, 0, 255), horizontal first, its uint8 result the input of the vertical one (the
//             clip between the passes is what a float two-pass misses: up to 19 grey levels on noise).
// The tap tables are built on the host in doubles (gill_clip_resize_taps exports the builder) and only for the outputs the crop keeps: `size`
// indices of the long axis from (new_long - size) / 2, all `size` of the short one.  Two launches: the horizontal pass writes the rows the kept
// output rows read into a uint8 intermediate in the caller's workspace, the vertical pass reads it and writes the normalised fp32 planes (and,
// on request, the cropped uint8 pixels).  Integer byte arithmetic, one thread per pixel (three channels), a few taps each: memory-bound and small.
#include "common.h"
#include "../../include/gill_amd.h"
#include <math.h>
#include <vector>

// the tap tables are compared word for word with a restatement in doubles: every operation below rounds on its own
#pragma clang fp contract(off)

static constexpr int kPrecisionBits = 22;      // Pillow's PRECISION_BITS for 8-bit channels: 32 - 8 - 2
static constexpr int kMaxEdge = 32768;         // per axis; keeps every product below in int32 / int64 range

static inline double cubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

static inline int taps_ksize(int in_size, int out_size) {
  const double scale = (double)in_size / (double)out_size;
  const double fs = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(2.0 * fs) * 2 + 1;
}

// xmin[i], n[i], k[i * i_stride + x * x_stride] for the outputs first .. first + count - 1 of an axis resampled in_size -> out_size; rows of k are
// zero-filled past n[i].  The order of the double operations is the contract (tests/clip_preprocess_util.py restates it): no contraction.
static void build_taps(int in_size, int out_size, int first, int count, int32_t* xmin_out, int32_t* n_out, int32_t* k_out, int64_t x_stride,
                       int64_t i_stride) {
  const double scale = (double)in_size / (double)out_size;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fs;
  std::vector<double> w((size_t)taps_ksize(in_size, out_size));
  for (int i = 0; i < count; ++i) {
    const double center = ((first + i) + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    const int n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      w[x] = cubic_filter((x + xmin - center + 0.5) / fs);
      ww += w[x];
    }
    for (int x = 0; x < n; ++x) {
      const double v = ww != 0.0 ? w[x] / ww : w[x];
      k_out[i * i_stride + x * x_stride] = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << kPrecisionBits)) : (int32_t)(0.5 + v * (double)(1 << kPrecisionBits));
    }
    xmin_out[i] = xmin;
    n_out[i] = n;
  }
}

extern "C" int gill_clip_resize_ksize(int in_size, int out_size) {
  if (in_size < 1 || out_size < 1 || in_size > kMaxEdge || out_size > kMaxEdge) return 0;
  return taps_ksize(in_size, out_size);
}

extern "C" int gill_clip_resize_taps(int in_size, int out_size, int first, int count, int32_t* xmin_out, int32_t* n_out, int32_t* k_out,
                                     int k_stride) {
  GILL_REQUIRE(xmin_out && n_out && k_out, "null argument");
  GILL_REQUIRE(in_size >= 1 && in_size <= kMaxEdge && out_size >= 1 && out_size <= kMaxEdge, "axis length out of range");
  GILL_REQUIRE(first >= 0 && count >= 1 && first <= out_size - count, "output window outside the axis");
  GILL_REQUIRE(k_stride >= taps_ksize(in_size, out_size), "k_stride below gill_clip_resize_ksize(in_size, out_size)");
  for (int64_t j = 0; j < (int64_t)count * k_stride; ++j) k_out[j] = 0;
  build_taps(in_size, out_size, first, count, xmin_out, n_out, k_out, 1, k_stride);
  return 0;
}

// ---------------------------------------------------------------- the plan of one call
// Device tables are int32 words: per axis and image `size` window starts, `size` tap counts, then ksize x size coefficients, tap-major
// (k[x * size + i]: neighbouring threads, which hold neighbouring outputs, read neighbouring words).
struct PreImg {
  int64_t src;        // byte offset of the image in the packed input
  int64_t mid;        // byte offset of its intermediate (rows x size x 3 uint8) in the workspace
  int32_t W;          // input row length in pixels
  int32_t row_lo;     // first input row the kept output rows read
  int32_t rows;       // how many
  int32_t htab, vtab; // word offsets of the two tables in the workspace
};

struct PrePlan {
  std::vector<PreImg> img;
  std::vector<int32_t> tab;
  size_t tab_off = 0, mid_off = 0, total = 0;   // byte offsets in the workspace
  int max_rows = 0;
};

static inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

static int make_plan(const int64_t* meta, int n, int size, int64_t packed_bytes, bool tables, PrePlan* p) {
  GILL_REQUIRE(meta && n >= 1 && n <= 65535, "1 .. 65535 images per call");
  GILL_REQUIRE(size >= 1 && size <= 4096, "size out of range");
  p->img.resize((size_t)n);
  size_t words = 0, mid = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t off = meta[3 * i], H = meta[3 * i + 1], W = meta[3 * i + 2];
    GILL_REQUIRE(H >= 1 && H <= kMaxEdge && W >= 1 && W <= kMaxEdge, "image edge out of range (1 .. 32768)");
    GILL_REQUIRE(off >= 0 && (packed_bytes < 0 || off + H * W * 3 <= packed_bytes), "image outside the packed buffer");
    // utils.ClipImageProcessor: shortest edge -> size, the long one int(size * long / short) (a Python float division, truncated)
    const int64_t shrt = W <= H ? W : H, lng = W <= H ? H : W;
    const int64_t new_long = (int64_t)((double)(size * lng) / (double)shrt);
    GILL_REQUIRE(new_long <= kMaxEdge, "resized long edge out of range");
    const int nw = W <= H ? size : (int)new_long, nh = W <= H ? (int)new_long : size;
    const int left = (nw - size) / 2, top = (nh - size) / 2;
    const int kh = taps_ksize((int)W, nw), kv = taps_ksize((int)H, nh);
    PreImg& d = p->img[(size_t)i];
    d.src = off;
    d.W = (int32_t)W;
    d.htab = (int32_t)words;
    words += (size_t)(2 + kh) * size;
    d.vtab = (int32_t)words;
    words += (size_t)(2 + kv) * size;
    GILL_REQUIRE(words < ((size_t)1 << 30), "tap tables too large");
    // the vertical windows of the kept rows grow monotonically: the first one's start and the last one's end bound what is read
    int32_t lo[1], cnt[1], hi[1];
    std::vector<int32_t> ktmp((size_t)kv);
    build_taps((int)H, nh, top, 1, lo, cnt, ktmp.data(), 1, kv);
    build_taps((int)H, nh, top + size - 1, 1, hi, cnt, ktmp.data(), 1, kv);
    d.row_lo = lo[0];
    d.rows = hi[0] + cnt[0] - lo[0];
    GILL_REQUIRE(d.rows >= 1 && d.row_lo >= 0 && d.row_lo + d.rows <= H, "internal: vertical window outside the image");
    d.mid = (int64_t)mid;
    mid += align256((size_t)d.rows * size * 3);
    if (d.rows > p->max_rows) p->max_rows = d.rows;
    if (tables) {
      p->tab.resize(words, 0);
      int32_t* h = p->tab.data() + d.htab;
      build_taps((int)W, nw, left, size, h, h + size, h + 2 * size, size, 1);
      int32_t* v = p->tab.data() + d.vtab;
      build_taps((int)H, nh, top, size, v, v + size, v + 2 * size, size, 1);
      for (int o = 0; o < size; ++o) {
        GILL_REQUIRE(h[o] >= 0 && h[o] + h[size + o] <= W && h[size + o] <= kh, "internal: horizontal window outside the image");
        GILL_REQUIRE(v[o] >= d.row_lo && v[o] + v[size + o] <= d.row_lo + d.rows && v[size + o] <= kv, "internal: vertical window outside the rows kept");
      }
    }
  }
  p->tab_off = align256(sizeof(PreImg) * (size_t)n);
  p->mid_off = align256(p->tab_off + words * sizeof(int32_t));
  p->total = p->mid_off + mid;
  return 0;
}

// ---------------------------------------------------------------- kernels
__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> kPrecisionBits;      // arithmetic shift, as Pillow's clip8
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// mid[img][r][o][c] = horizontal pass of input row row_lo + r at kept output column o
__global__ __launch_bounds__(256) void clip_pre_horizontal_kernel(const uint8_t* __restrict__ packed, const PreImg* __restrict__ imgs,
                                                                   const int32_t* __restrict__ tabs, int size, uint8_t* __restrict__ mid) {
  const PreImg d = imgs[blockIdx.y];
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= d.rows * size) return;
  const int r = p / size, o = p - r * size;
  const int32_t* tab = tabs + d.htab;
  const int xmin = tab[o], n = tab[size + o];
  const int32_t* k = tab + 2 * size + o;
  const uint8_t* src = packed + d.src + ((int64_t)(d.row_lo + r) * d.W + xmin) * 3;
  int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
  for (int x = 0; x < n; ++x) {
    const int kk = k[(size_t)x * size];
    a0 += kk * src[3 * x];
    a1 += kk * src[3 * x + 1];
    a2 += kk * src[3 * x + 2];
  }
  uint8_t* dst = mid + d.mid + ((int64_t)r * size + o) * 3;
  dst[0] = (uint8_t)clip8(a0);
  dst[1] = (uint8_t)clip8(a1);
  dst[2] = (uint8_t)clip8(a2);
}

struct PreNorm { float scale, mean[3], std[3]; };

// vertical pass over the intermediate at kept output row y, then (u8 * (1 / 255) - mean) / std into plane c of out[img]: three separately
// rounded fp32 operations, as numpy does them in utils.ClipImageProcessor
__global__ __launch_bounds__(256) void clip_pre_vertical_kernel(const uint8_t* __restrict__ mid, const PreImg* __restrict__ imgs,
                                                                 const int32_t* __restrict__ tabs, int size, PreNorm nm, float* __restrict__ out,
                                                                 uint8_t* __restrict__ out_u8) {
  const PreImg d = imgs[blockIdx.y];
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= size * size) return;
  const int y = p / size, o = p - y * size;
  const int32_t* tab = tabs + d.vtab;
  const int ymin = tab[y], n = tab[size + y];
  const int32_t* k = tab + 2 * size + y;
  const size_t pitch = (size_t)size * 3;
  const uint8_t* src = mid + d.mid + (size_t)(ymin - d.row_lo) * pitch + (size_t)o * 3;
  int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
  for (int t = 0; t < n; ++t) {
    const int kk = k[(size_t)t * size];
    a0 += kk * src[t * pitch];
    a1 += kk * src[t * pitch + 1];
    a2 += kk * src[t * pitch + 2];
  }
  const int v[3] = {clip8(a0), clip8(a1), clip8(a2)};
  const size_t plane = (size_t)size * size;
  float* op = out + (size_t)blockIdx.y * 3 * plane + p;
#pragma unroll
  for (int c = 0; c < 3; ++c) op[c * plane] = __fdiv_rn(__fsub_rn(__fmul_rn((float)v[c], nm.scale), nm.mean[c]), nm.std[c]);
  if (out_u8) {
    uint8_t* up = out_u8 + ((size_t)blockIdx.y * plane + p) * 3;
    up[0] = (uint8_t)v[0];
    up[1] = (uint8_t)v[1];
    up[2] = (uint8_t)v[2];
  }
}

// ---------------------------------------------------------------- entry points
extern "C" int gill_clip_preprocess_workspace(const int64_t* meta_host, int n, int size, int64_t* bytes_out) {
  GILL_REQUIRE(bytes_out, "null argument");
  PrePlan p;
  GILL_TRY(make_plan(meta_host, n, size, -1, false, &p));
  *bytes_out = (int64_t)p.total;
  return 0;
}

extern "C" int gill_clip_preprocess(const uint8_t* packed, int64_t packed_bytes, const int64_t* meta_host, int n, int size, int crop_size,
                                    float* out, uint8_t* out_u8, void* workspace, int64_t workspace_bytes, void* stream) {
  GILL_REQUIRE(packed && out && workspace && packed_bytes >= 0, "null argument");
  GILL_REQUIRE(size == crop_size, "only size == crop_size (what every openai/clip-vit-* feature extractor uses) is built");
  GILL_REQUIRE((uintptr_t)workspace % 8 == 0, "workspace must be 8-byte aligned");
  PrePlan p;
  GILL_TRY(make_plan(meta_host, n, size, packed_bytes, true, &p));
  GILL_REQUIRE(workspace_bytes >= (int64_t)p.total, "workspace below gill_clip_preprocess_workspace()");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)workspace;
  GILL_CHECK_HIP(hipMemcpyAsync(ws, p.img.data(), sizeof(PreImg) * p.img.size(), hipMemcpyHostToDevice, s));
  GILL_CHECK_HIP(hipMemcpyAsync(ws + p.tab_off, p.tab.data(), sizeof(int32_t) * p.tab.size(), hipMemcpyHostToDevice, s));
  GILL_CHECK_HIP(hipStreamSynchronize(s));   // the plan is a call-lifetime host buffer
  const PreImg* imgs = (const PreImg*)ws;
  const int32_t* tabs = (const int32_t*)(ws + p.tab_off);
  uint8_t* mid = ws + p.mid_off;
  // utils.ClipImageProcessor: np.float32(1.0 / 255.0), image_mean, image_std as float32
  const PreNorm nm = {(float)(1.0 / 255.0), {0.48145466f, 0.4578275f, 0.40821073f}, {0.26862954f, 0.26130258f, 0.27577711f}};
  hipLaunchKernelGGL(clip_pre_horizontal_kernel, dim3(cdiv(p.max_rows * size, 256), n), dim3(256), 0, s, packed, imgs, tabs, size, mid);
  GILL_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(clip_pre_vertical_kernel, dim3(cdiv(size * size, 256), n), dim3(256), 0, s, (const uint8_t*)mid, imgs, tabs, size, nm, out,
                     out_u8);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}
