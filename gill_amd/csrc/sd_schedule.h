// Host-only scheduler arithmetic of the SD denoise loop (sd_schedule.hip): what sd_denoise_on (unet.hip) and the sampler operator entry
// (unet_ops.hip) build their device tables from.  The C entries gill_pndm_schedule / gill_sd_schedule(_from) / gill_sd_inpaint_keep sit on top.
#pragma once
#include "../../include/gill_amd.h"
#include "ops.h"
#include <vector>

enum { SD_PNDM = 0, SD_DDIM = 1, SD_DPMPP_2M = 2, SD_EULER = 3, SD_EULER_A = 4 };
struct SdSchedule {
  int kind = 0;
  std::vector<float> timesteps;       // one per UNet call, as the time embedding sees them
  double init_noise_sigma = 1.0;
  std::vector<PlmsRow> plms;          // kind 0
  std::vector<SamplerRow> rows;       // every other kind
  bool needs_noise = false;           // some row has c_n != 0
  double add_a = 1.0, add_b = 0.0;    // the scheduler's add_noise() at the first timestep: x_start = add_a * init_latents + add_b * noise
};
// Both hidden, as when they were static in unet.hip: their mangled names carry gill_sd_sampler and would otherwise join the exported gill_* names.
// start > 0: the loop begins at step `start` of the schedule (sd_schedule.hip)
__attribute__((visibility("hidden"))) int sd_schedule(const gill_sd_sampler* sp, bool vpred, int num_steps, SdSchedule& out, int start = 0);
// blend-mode inpainting: keep [ncalls][2], the add_noise pair at the noise level the latents have after each call of `sched`
__attribute__((visibility("hidden"))) int sd_inpaint_keep(const gill_sd_sampler* sp, bool vpred, int num_steps, int start, const SdSchedule& sched,
                                                          std::vector<double>& keep);
