// The denoise loop's scheduler arithmetic (sd_schedule.h): timesteps and per-call coefficient rows of every sampler.  Host only: nothing here touches the device.
#include "sd_schedule.h"

// PNDM (PLMS, skip_prk_steps=True, steps_offset=1, scaled_linear betas 0.00085..0.012 over 1000 train steps).
static void pndm_alphas_cumprod(std::vector<float>& ac) {
  const int T = 1000;
  ac.resize(T);
  const float a = sqrtf(0.00085f), b = sqrtf(0.012f);
  const float step = (b - a) / (float)(T - 1);
  float prod = 1.f;
  for (int i = 0; i < T; ++i) {
    // torch.linspace (fp32): symmetric evaluation around the midpoint
    const float v = (i < T / 2) ? a + step * (float)i : b - step * (float)(T - 1 - i);
    const float beta = v * v;
    prod *= (1.f - beta);
    ac[i] = prod;
  }
}
static void pndm_timesteps(int num_steps, std::vector<int>& ts, int* ratio_out, int steps_offset = 1) {
  const int ratio = 1000 / num_steps;
  std::vector<int> base(num_steps);
  for (int i = 0; i < num_steps; ++i) base[i] = i * ratio + steps_offset;   // (1 for SD)
  // plms_timesteps = concat(base[:-1], base[-2:-1], base[-1:])[::-1]
  std::vector<int> seq(base.begin(), base.end() - 1);
  if (num_steps >= 2) seq.push_back(base[num_steps - 2]);
  seq.push_back(base[num_steps - 1]);
  ts.assign(seq.rbegin(), seq.rend());
  *ratio_out = ratio;
}

extern "C" int gill_pndm_schedule(int num_steps, int32_t* timesteps_out, double* alphas_cumprod_out) {
  GILL_REQUIRE(num_steps >= 2 && num_steps <= 1000, "num_steps out of range");
  std::vector<int> ts; int ratio;
  pndm_timesteps(num_steps, ts, &ratio);
  if (timesteps_out) for (size_t i = 0; i < ts.size(); ++i) timesteps_out[i] = ts[i];
  if (alphas_cumprod_out) {
    std::vector<float> ac; pndm_alphas_cumprod(ac);
    for (int i = 0; i < 1000; ++i) alphas_cumprod_out[i] = (double)ac[i];
  }
  return (int)ts.size();
}

// the PLMS schedule of every call (host arithmetic in double, like the scheduler's numpy/torch-CPU tables)
static void pndm_rows(const std::vector<int>& ts, int ratio, const std::vector<float>& ac, bool v_prediction, bool set_alpha_to_one,
                      std::vector<PlmsRow>& rows) {
  const int ncalls = (int)ts.size();
  rows.resize(ncalls);
  int counter = 0, n_ets = 0, last = -1;
  for (int i = 0; i < ncalls; ++i) {
    int t = ts[i];
    int prev_t = t - ratio;
    PlmsRow& a = rows[i];
    a.slot_new = -1; a.s1 = a.s2 = a.s3 = 0;
    if (counter != 1) {
      a.slot_new = (last + 1) & 3;
      a.s1 = last & 3; a.s2 = (last + 3) & 3; a.s3 = (last + 2) & 3;
      last = a.slot_new;
      if (n_ets < 4) ++n_ets;
    } else {
      prev_t = t; t = t + ratio;
      a.s1 = last & 3;
    }
    if (n_ets == 1 && counter == 0) a.mode = 0;
    else if (n_ets == 1 && counter == 1) a.mode = 1;
    else if (n_ets == 2) a.mode = 2;
    else if (n_ets == 3) a.mode = 3;
    else a.mode = 4;
    // _get_prev_sample
    const double at = ac[t];
    const double ap = prev_t >= 0 ? (double)ac[prev_t] : (set_alpha_to_one ? 1.0 : (double)ac[0]);   // (False for SD)
    const double bt = 1.0 - at, bp = 1.0 - ap;
    const double sample_coeff = sqrt(ap / at);
    const double denom = at * sqrt(bp) + sqrt(at * bt * ap);
    double sc = sample_coeff, ec = (ap - at) / denom;
    if (v_prediction) {   // the model output is v: eps' = sqrt(a_t) v + sqrt(1 - a_t) sample, folded into the two coefficients
      sc -= ec * sqrt(bt);
      ec *= sqrt(at);
    }
    a.sample_coeff = (float)sc;
    a.eps_coeff = (float)ec;
    ++counter;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// The linear samplers (diffusers 0.17.1 as configured for SD: scaled_linear betas, no clipping / thresholding / Karras sigmas).  Every table is
// built in double from the fp32 alphas_cumprod above and rounded to fp32 once, into SamplerRow.

// np.linspace(0, 999, num): arange(num) * step, the last element set to the end point
static void linspace_999(int num, std::vector<double>& v) {
  v.resize(num);
  const double step = num > 1 ? 999.0 / (double)(num - 1) : 0.0;
  for (int i = 0; i < num; ++i) v[i] = (double)i * step;
  if (num > 1) v[num - 1] = 999.0;
}

// start (image-to-image, include/gill_amd.h gill_sd_schedule_from): the loop begins at step `start` of the num_steps schedule.  start == 0 is the
// text-to-image table, bit for bit.
//   ddim, euler, euler_ancestral: the tail of the full table;
//   dpmsolver++: the tail, its first row a first-order step (the solver's history is empty, as diffusers' scheduler starts); ring slots keep the
//     full table's parity, so the rows that follow read the slot the rebuilt row wrote;
//   pndm: the PLMS warm-up pair replayed at t_s: t_s, t_s - D, t_s - D, t_s - 2D, ... (num_steps - start + 1 calls).  DELIBERATELY not what
//     diffusers 0.17's img2img does (it slices the already-duplicated list, so that from the third call on the model is evaluated one grid step
//     ahead of the latents): this is the warm-up a fresh run on the same grid makes from t_s.  With start == num_steps - 1 the second timestep
//     falls below the grid's end: the coefficients then use the final alpha (as every step below t = 0 does) and the model sees t = 0.
int sd_schedule(const gill_sd_sampler* sp, bool vpred, int num_steps, SdSchedule& out, int start) {
  GILL_REQUIRE(sp != nullptr, "null sampler");
  GILL_REQUIRE(sp->kind >= SD_PNDM && sp->kind <= SD_EULER_A, "unknown sampler kind (0 pndm, 1 ddim, 2 dpmsolver++, 3 euler, 4 euler_ancestral)");
  out.kind = sp->kind;
  std::vector<float> ac; pndm_alphas_cumprod(ac);
  const int T = 1000;
  if (sp->kind == SD_PNDM) {
    GILL_REQUIRE(num_steps >= 2 && num_steps <= 1000, "num_steps out of range");
    GILL_REQUIRE(sp->steps_offset >= 0, "pndm: steps_offset must be >= 0");
    GILL_REQUIRE((num_steps - 1) * (T / num_steps) + sp->steps_offset < T, "pndm: num_steps and steps_offset put a timestep past the training range");
    GILL_REQUIRE(start >= 0 && start < num_steps, "start must be in [0, num_steps)");
    std::vector<int> ts; int ratio;
    pndm_timesteps(num_steps, ts, &ratio, sp->steps_offset);
    if (start > 0) {
      // ts = [t_0, t_1, t_1, t_2, ...]: grid point k >= 1 sits at index k + 1
      std::vector<int> tail;
      const int ts_s = ts[start + 1];
      tail.push_back(ts_s); tail.push_back(ts_s - ratio); tail.push_back(ts_s - ratio);
      for (size_t k = (size_t)start + 3; k < ts.size(); ++k) tail.push_back(ts[k]);
      tail.resize((size_t)(num_steps - start + 1));      // (start == num_steps - 1: the pair only)
      ts.swap(tail);
    }
    pndm_rows(ts, ratio, ac, vpred, sp->set_alpha_to_one != 0, out.plms);
    out.timesteps.resize(ts.size());
    for (size_t i = 0; i < ts.size(); ++i) out.timesteps[i] = (float)(ts[i] > 0 ? ts[i] : 0);
    out.add_a = sqrt((double)ac[ts[0]]); out.add_b = sqrt(1.0 - (double)ac[ts[0]]);
    return 0;
  }
  GILL_REQUIRE(num_steps >= 1 && num_steps <= 1000, "num_steps out of range");
  GILL_REQUIRE(start >= 0 && start < num_steps, "start must be in [0, num_steps)");
  const int N = num_steps;
  out.rows.assign(N, SamplerRow{-1, 0, 1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f});
  out.timesteps.resize(N);
  auto put = [&](int i, int slot_new, int s1, double in_scale, double p_x, double p_e, double c_x, double c_0, double c_1, double c_n) {
    out.rows[i] = SamplerRow{slot_new, s1, (float)in_scale, (float)p_x, (float)p_e, (float)c_x, (float)c_0, (float)c_1, (float)c_n};
  };
  if (sp->kind == SD_DDIM) {
    GILL_REQUIRE(sp->eta >= 0.f, "ddim: eta must be >= 0");     // (a NaN fails this too)
    GILL_REQUIRE(sp->steps_offset >= 0, "ddim: steps_offset must be >= 0");
    const int r = T / N;
    GILL_REQUIRE((N - 1) * r + sp->steps_offset < T, "ddim: num_steps and steps_offset put a timestep past the training range");
    for (int i = 0; i < N; ++i) {
      const int t = (N - 1 - i) * r + sp->steps_offset, prev = t - r;
      const double at = ac[t], ap = prev >= 0 ? (double)ac[prev] : (sp->set_alpha_to_one ? 1.0 : (double)ac[0]);
      const double sd = (double)sp->eta * sqrt((1.0 - ap) / (1.0 - at)) * sqrt(1.0 - at / ap);
      const double dir = sqrt(1.0 - ap - sd * sd);
      // m = eps;  x0 = (x - sqrt(1 - a_t) eps) / sqrt(a_t);  x_prev = sqrt(a_p) x0 + dir eps + sd z
      put(i, -1, 0, 1.0, vpred ? sqrt(1.0 - at) : 0.0, vpred ? sqrt(at) : 1.0, sqrt(ap / at), dir - sqrt(ap) * sqrt(1.0 - at) / sqrt(at), 0.0, sd);
      out.timesteps[i] = (float)t;
      if (i == start) { out.add_a = sqrt(at); out.add_b = sqrt(1.0 - at); }
    }
  } else if (sp->kind == SD_DPMPP_2M) {
    GILL_REQUIRE(N <= 999, "dpmsolver++: num_steps above 999 repeats a timestep");
    std::vector<double> ls; linspace_999(N + 1, ls);
    std::vector<int> ts(N + 1);       // ts[N] = 0: the target of the last call
    for (int i = 0; i < N; ++i) ts[i] = (int)rint(ls[N - i]);     // np.round: half to even
    ts[N] = 0;
    auto alpha = [&](int t) { return sqrt((double)ac[t]); };
    auto sigma = [&](int t) { return sqrt(1.0 - (double)ac[t]); };
    auto lambda = [&](int t) { return log(alpha(t)) - log(sigma(t)); };
    for (int i = 0; i < N; ++i) {
      const int s0 = ts[i], t = ts[i + 1];
      const double h = lambda(t) - lambda(s0), E = exp(-h) - 1.0;
      const double p_x = vpred ? alpha(s0) : 1.0 / alpha(s0), p_e = vpred ? -sigma(s0) : -sigma(s0) / alpha(s0);   // m = x0
      const bool first_order = i <= start || (i == N - 1 && N < 15);    // empty history (rows before `start` are dropped below; i = 0 has no ts[i - 1]); lower_order_final (decided on the FULL schedule's length)
      double c_0 = -alpha(t) * E, c_1 = 0.0;
      if (!first_order) {
        const double r0 = (lambda(s0) - lambda(ts[i - 1])) / h;
        c_0 = -alpha(t) * E * (1.0 + 0.5 / r0);       // D1 = (m0 - m1) / r0
        c_1 = 0.5 * alpha(t) * E / r0;
      }
      put(i, i & 1, (i + 1) & 1, 1.0, p_x, p_e, sigma(t) / sigma(s0), c_0, c_1, 0.0);
      out.timesteps[i] = (float)s0;
      if (i == start) { out.add_a = alpha(s0); out.add_b = sigma(s0); }
    }
  } else {   // Euler, Euler ancestral
    std::vector<double> ls; linspace_999(N, ls);
    std::vector<double> sg(N + 1);
    double smax = 0.0;
    for (int i = 0; i < N; ++i) {
      const double t = ls[N - 1 - i];
      int j = (int)floor(t); if (j > T - 2) j = T - 2;
      const double f0 = sqrt((1.0 - (double)ac[j]) / (double)ac[j]), f1 = sqrt((1.0 - (double)ac[j + 1]) / (double)ac[j + 1]);
      sg[i] = (f1 - f0) * (t - (double)j) + f0;      // np.interp
      if (sg[i] > smax) smax = sg[i];
      out.timesteps[i] = (float)t;
    }
    sg[N] = 0.0;
    out.init_noise_sigma = smax;
    out.add_a = 1.0; out.add_b = sg[start];
    for (int i = 0; i < N; ++i) {
      const double s = sg[i], to = sg[i + 1], q = s * s + 1.0;
      // m = eps;  v-prediction: x0 = x / (s^2 + 1) - v s / sqrt(s^2 + 1), eps = (x - x0) / s
      const double p_x = vpred ? s / q : 0.0, p_e = vpred ? 1.0 / sqrt(q) : 1.0;
      if (sp->kind == SD_EULER) put(i, -1, 0, 1.0 / sqrt(q), p_x, p_e, 1.0, to - s, 0.0, 0.0);
      else {
        const double up = sqrt(to * to * (s * s - to * to) / (s * s)), down = sqrt(to * to - up * up);
        put(i, -1, 0, 1.0 / sqrt(q), p_x, p_e, 1.0, down - s, 0.0, up);
      }
    }
  }
  if (start > 0) {
    out.rows.erase(out.rows.begin(), out.rows.begin() + start);
    out.timesteps.erase(out.timesteps.begin(), out.timesteps.begin() + start);
  }
  for (const SamplerRow& r : out.rows) {
    const float v[7] = {r.in_scale, r.p_x, r.p_e, r.c_x, r.c_0, r.c_1, r.c_n};
    for (float f : v) GILL_REQUIRE(std::isfinite(f), "sampler table: a coefficient is not finite for these arguments");
    if (r.c_n != 0.f) out.needs_noise = true;
  }
  return 0;
}

extern "C" int gill_sd_schedule_from(const gill_sd_sampler* sampler, int v_prediction, int num_steps, int start, float* timesteps_out,
                                     double* init_noise_sigma_out, double* rows_out, double* add_noise_out) {
  SdSchedule sc;
  GILL_TRY(sd_schedule(sampler, v_prediction != 0, num_steps, sc, start));
  if (add_noise_out) { add_noise_out[0] = sc.add_a; add_noise_out[1] = sc.add_b; }
  const int ncalls = (int)sc.timesteps.size();
  if (timesteps_out) for (int i = 0; i < ncalls; ++i) timesteps_out[i] = sc.timesteps[i];
  if (init_noise_sigma_out) *init_noise_sigma_out = sc.init_noise_sigma;
  if (rows_out) {
    for (int i = 0; i < ncalls; ++i) {
      double* o = rows_out + (size_t)i * GILL_SD_ROW_DOUBLES;
      for (int k = 0; k < GILL_SD_ROW_DOUBLES; ++k) o[k] = 0.0;
      if (sc.kind == SD_PNDM) {
        const PlmsRow& r = sc.plms[i];
        o[0] = r.mode; o[1] = r.slot_new; o[2] = r.s1; o[3] = r.s2; o[4] = r.s3;
        o[5] = 1.0; o[7] = 1.0; o[8] = r.sample_coeff; o[9] = -(double)r.eps_coeff;
      } else {
        const SamplerRow& r = sc.rows[i];
        o[0] = -1.0; o[1] = r.slot_new; o[2] = r.s1;
        o[5] = r.in_scale; o[6] = r.p_x; o[7] = r.p_e; o[8] = r.c_x; o[9] = r.c_0; o[10] = r.c_1; o[11] = r.c_n;
      }
    }
  }
  return ncalls;
}
extern "C" int gill_sd_schedule(const gill_sd_sampler* sampler, int v_prediction, int num_steps, float* timesteps_out,
                                double* init_noise_sigma_out, double* rows_out) {
  return gill_sd_schedule_from(sampler, v_prediction, num_steps, 0, timesteps_out, init_noise_sigma_out, rows_out, nullptr);
}

// Inpainting, blend mode: the add_noise pair (ka, kb) at the noise level the latents have AFTER call i of the table sd_schedule(..., start) builds,
// so that ka * x0 + kb * z0 is the image at that level.  i < ncalls - 1: the pair at the timestep of call i + 1 (for the linear kinds that equals
// sd_schedule's own add_noise pair at start + i + 1, built here from the same values without a table per step; for pndm sqrt(abar), sqrt(1 - abar) at the table's timestep i + 1, which repeats after the
// warm-up pair: calls 0 and 1 both leave the latents at t_s - D).  The last call leaves the clean latents: (1, 0).
int sd_inpaint_keep(const gill_sd_sampler* sp, bool vpred, int num_steps, int start, const SdSchedule& sched, std::vector<double>& keep) {
  const int ncalls = (int)sched.timesteps.size();
  keep.assign((size_t)ncalls * 2, 0.0);
  std::vector<float> ac; pndm_alphas_cumprod(ac);
  std::vector<double> ls;
  const bool euler = sched.kind == SD_EULER || sched.kind == SD_EULER_A;
  if (euler) linspace_999(num_steps, ls);
  for (int i = 0; i + 1 < ncalls; ++i) {
    if (euler) {      // (1, sigma of full-table step start + i + 1), interpolated as sd_schedule does
      const double t = ls[num_steps - 1 - (start + i + 1)];
      int j = (int)floor(t); if (j > 998) j = 998;
      const double f0 = sqrt((1.0 - (double)ac[j]) / (double)ac[j]), f1 = sqrt((1.0 - (double)ac[j + 1]) / (double)ac[j + 1]);
      keep[2 * i] = 1.0; keep[2 * i + 1] = (f1 - f0) * (t - (double)j) + f0;
    } else {          // pndm, ddim, dpmsolver++: integer timesteps (pndm's clamped at 0, as the table's are)
      const double at = ac[(int)sched.timesteps[i + 1]];
      keep[2 * i] = sqrt(at); keep[2 * i + 1] = sqrt(1.0 - at);
    }
  }
  keep[2 * (ncalls - 1)] = 1.0; keep[2 * (ncalls - 1) + 1] = 0.0;
  return 0;
}
extern "C" int gill_sd_inpaint_keep(const gill_sd_sampler* sampler, int v_prediction, int num_steps, int start, double* keep_out) {
  SdSchedule sc;
  GILL_TRY(sd_schedule(sampler, v_prediction != 0, num_steps, sc, start));
  std::vector<double> keep;
  GILL_TRY(sd_inpaint_keep(sampler, v_prediction != 0, num_steps, start, sc, keep));
  if (keep_out) for (size_t i = 0; i < keep.size(); ++i) keep_out[i] = (double)(float)keep[i];     // the fp32 values the device reads, widened
  return (int)sc.timesteps.size();
}
