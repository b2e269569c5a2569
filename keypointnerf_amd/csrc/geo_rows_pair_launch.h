// geo_rows_pair_launch.h — the launchers of geo_rows_pair_kernels.hip, defined once: included by geo_rows_pair_tu.hip (device build)
// and by kpn_api.hip (emulator build, one translation unit).  Not part of the C ABI: run_field (api_field.hip) calls them with its grids.
#pragma once
#define KPN_PAIR_LAUNCHER extern "C" __attribute__((visibility("hidden"))) void

// the rows of one batch, rows modes 2 and 3
KPN_PAIR_LAUNCHER kpn_internal_launch_geo_rows_pair(int mode, int blocks, void* stream, const kpn_scene_dev* sc, const kpn_points* ps, const float* wp,
                                                    const int* list, const int* count, int* tickets, float* xscr, const kpn_batch* batch) {
    if (batch->pool) {   // pooling over the views inside the kernel (POOL layout of the scratch)
        if (mode == 3) KPN_LAUNCH(k_geo_rows_f2p, dim3(blocks), dim3(256), stream, *sc, *ps, wp, list, count, tickets, xscr, *batch);
        else KPN_LAUNCH(k_geo_rows_h2p, dim3(blocks), dim3(256), stream, *sc, *ps, wp, list, count, tickets, xscr, *batch);
    } else if (mode == 3)
        KPN_LAUNCH(k_geo_rows_f2, dim3(blocks), dim3(256), stream, *sc, *ps, wp, list, count, tickets, xscr, *batch);
    else
        KPN_LAUNCH(k_geo_rows_h2, dim3(blocks), dim3(256), stream, *sc, *ps, wp, list, count, tickets, xscr, *batch);
}
// the gather records of the same batch (the pair-tile kernels do not write them)
KPN_PAIR_LAUNCHER kpn_internal_launch_row_records(int blocks, void* stream, const kpn_scene_dev* sc, const kpn_points* ps, const float* wp, const int* list,
                                                  const int* count, float* xscr, const kpn_batch* batch) {
    KPN_LAUNCH(k_row_records, dim3(blocks), dim3(256), stream, *sc, *ps, wp, list, count, xscr, *batch);
}
// ... of the batch's live points only (density-first render passes)
KPN_PAIR_LAUNCHER kpn_internal_launch_row_records_live(int blocks, void* stream, const kpn_scene_dev* sc, const kpn_points* ps, const float* wp,
                                                       const int* list, const int* count, const int* tickets, const int* live, float* xscr,
                                                       const kpn_batch* batch) {
    KPN_LAUNCH(k_row_records_live, dim3(blocks), dim3(256), stream, *sc, *ps, wp, list, count, tickets, live, xscr, *batch);
}
#undef KPN_PAIR_LAUNCHER
