// Translation unit of k_geo_rows_h2 (geo_rows_pair_kernels.hip) for the device build: compiled with -fno-slp-vectorize.
// The kernel's VALU work is interleaved with its MFMAs by hand; the SLP vectoriser gathers those scalar operations into
// packed-f32 lumps (v_pk_mul_f32 ...) placed ahead of the MFMAs they were meant to sit between (measured: 7.4 -> 6.8 ms per
// launch without it), and packed f32 VALU is an anti-lever beside MFMAs anyway (MI355X_MICROARCH.md).  The flag changes
// the rounding of other kernels' contracted arithmetic, so it is confined to this file; the rest of the library is
// kpn_api.hip.  The host emulator build includes the kernel and its launchers into kpn_api.hip directly (one translation unit, no flags).
#include "kpn_field_shared.h"
#include "geo_rows_pair_kernels.hip"

#include "geo_rows_pair_launch.h"   // kpn_internal_launch_*: what run_field (api_field.hip) calls for rows modes 2 and 3

#ifdef KPN_PRECISION_PROBE
extern "C" __attribute__((visibility("hidden"))) int kpn_internal_probe_set_mask_pair(unsigned long long m) {
    return hipMemcpyToSymbol(HIP_SYMBOL(kpn_probe_mask_dev), &m, sizeof(m)) != hipSuccess;
}
#endif
#ifdef KPN_H2_TIMING
// debug builds only: read (and clear) the per-phase cycle sums of k_geo_rows_h2
extern "C" int kpn_h2_timing(unsigned long long* out8) {
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(kpn_h2_cycles), 64) != hipSuccess) return 1;
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(kpn_h2_cycles), z, 64) != hipSuccess;
}
#endif
