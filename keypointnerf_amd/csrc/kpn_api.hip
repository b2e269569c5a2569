// kpn_api.hip — C ABI (include/kpnerf.h): the translation unit's table of contents.  The kernels, then the host parts
// (api_*.hip) in dependency order.  Host code only launches kernels on the caller's stream; it never
// synchronises or allocates (except kpn_selftest_mfma, a diagnostic).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/kpnerf.h"
#include "kpn_device.h"
#include "kpn_reduce.h"

// kernels (ray_kernels.hip / field_kernels.hip)
#include "ray_kernels.hip"
#include "field_kernels.hip"
#ifdef KPN_SIMT_EMU
#include "geo_rows_pair_kernels.hip"   // the device build compiles this kernel as its own translation unit (geo_rows_pair_tu.hip)
#include "geo_rows_pair_launch.h"      // ... with these launchers, which the device build only declares:
#else
extern "C" void kpn_internal_launch_row_records(int blocks, void* stream, const kpn_scene_dev* sc, const kpn_points* ps, const float* wp, const int* list,
                                                const int* count, float* xscr, const kpn_batch* batch);
extern "C" void kpn_internal_launch_row_records_live(int blocks, void* stream, const kpn_scene_dev* sc, const kpn_points* ps, const float* wp,
                                                     const int* list, const int* count, const int* tickets, const int* live, float* xscr,
                                                     const kpn_batch* batch);
extern "C" void kpn_internal_launch_geo_rows_pair(int mode, int blocks, void* stream, const kpn_scene_dev* sc, const kpn_points* ps, const float* wp,
                                                  const int* list, const int* count, int* tickets, float* xscr, const kpn_batch* batch);
#endif
#include "field_bwd_kernels.hip"
#include "fuse_bwd_kernels.hip"
#include "kpt_grad_kernels.hip"       // the keypoint gradient, from the dumps of field_bwd_kernels.hip
#include "vgg_kernels.hip"
#include "encoder_kernels.hip"
#include "encoder_split_kernels.hip"   // the stride-1 family on three bf16 pieces (KPN_CONV_BF16X3)
#include "loss_kernels.hip"
#include "param_kernels.hip"

// host parts
#include "api_common.h"
#include "api_profile.hip"    // before the parts that record into it
#include "api_weights.hip"
#include "api_scene.hip"
#include "api_field.hip"
#include "api_backward.hip"
#include "api_render.hip"
#include "api_metrics.hip"
#include "api_vgg.hip"
#include "api_encoders.hip"
#include "api_layer.hip"      // one convolution layer over the launch layer: the five files below name theirs
#include "api_conv.hip"
#include "api_strided.hip"
#include "api_reppad.hip"
#include "api_norm.hip"
#include "api_block.hip"
#include "api_tex_train.hip"
#include "api_resample.hip"
#include "api_geo_train.hip"  // the blocks, the layers and the resampling steps above as one HGFilterV2
#include "api_params.hip"

extern "C" int kpn_abi_version(void) { return KPN_ABI_VERSION; }
extern "C" const char* kpn_last_error(void) { return g_err.c_str(); }
extern "C" int kpn_is_device_build(void) {
#ifdef KPN_SIMT_EMU
    return 0;
#else
    return 1;
#endif
}
