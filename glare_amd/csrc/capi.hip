// Version / status entry points of libglare_hip.so.
#include "common.h"

extern "C" int glare_version(void) { return 131; }  // 1.31: + NIQE of unpaired results (glare_niqe_luma_u8, _mscn_f32, _block_moments_f32, _halve_f32)
                                                    // 1.30: + averaged weights (glare_weight_ema_f32, glare_swap_f32)
                                                    // 1.29: + semantic guidance (glare_vq_semantic_bf16, glare_vq_semantic_scale_f32)
                                                    // 1.28: + EMA codebook (glare_vq_ema_stats_f32, glare_vq_ema_update_f32, glare_vq_restart_ema_f32)
                                                    // 1.27: + codebook restart (glare_vq_restart_f32)
                                                    // 1.25: + tiled enhancement (glare_harness_tile_gather_u8, glare_harness_tile_blend_f32)
                                                    // 1.23: + the codebook layer's training form (glare_vq_loss_sum_f32, glare_vq_backward_f32)
                                                    // 1.21: + the unpaired harness (any-size pad / encode, uint8 post-process)
                                                    // 1.20: + IEEE-half twin library, hi / lo residual stream, grouped conv launches, single-pass DCN,
                                                    //       ActNorm initialisation, guarded Adam / GradScaler (1.10: training step, DCN v1, device-side harness)

extern "C" const char* glare_status_string(int status) {
  switch (status) {
    case GLARE_OK: return "ok";
    case GLARE_ERR_INVALID: return "invalid argument";
    case GLARE_ERR_LAUNCH: return "HIP launch failure";
    case GLARE_ERR_WORKSPACE: return "workspace too small";
    case GLARE_ERR_UNSUPPORTED: return "unsupported configuration";
    default: return "unknown status";
  }
}
