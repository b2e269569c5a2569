// ---------------------------------------------------------------------------------------------
// the parameter leg of a training step (param_kernels.hip): fold, fold backward, Adam.  The layer table is api_weights.hip's
// (plain_dims, plain_w_off, plain_b_off); what is added here is which of its layers the reference wraps in weight_norm
// (src/utils.py:542-543: every linear of MLPUNet but the last of each stack).
namespace {
const bool plain_normed[P_COUNT] = {true, true, true, false, true, true, false, false, false, false,
                                    false, false, false, false, false, false, false, false, false};
int fold_norm_rows() { int n = 0; for (int l = 0; l < P_COUNT; ++l) if (plain_normed[l]) n += plain_dims[l][0]; return n; }
int fold_rows() { int n = 0; for (int l = 0; l < P_COUNT; ++l) n += plain_dims[l][0]; return n; }
void fold_layers(kpn_fold_kargs& k) {
    int row = 0, norm = 0;
    for (int l = 0; l < P_COUNT; ++l) {
        k.layer[l] = {row, plain_dims[l][1], (int)plain_w_off(l), (int)plain_b_off(l), plain_normed[l] ? norm : -1};
        row += plain_dims[l][0];
        if (plain_normed[l]) norm += plain_dims[l][0];
    }
    k.ani_off = (int)plain_w_off(P_COUNT);
}
// norms: [normed rows] fp64 n, then [normed rows] fp32 s
void fold_bind_norms(kpn_fold_kargs& k, float* norms) {
    k.norm_n = reinterpret_cast<double*>(norms);
    k.norm_s = norms + 2 * (size_t)fold_norm_rows();
}
}  // namespace
static_assert(KPN_PARAM_LAYERS == P_COUNT, "kpn_param_table has one entry per layer of the plain layout");

static int check_field_shape(const kpn_field_shape* s) {
    KPN_REQUIRE(s != nullptr, "null field shape");
    KPN_REQUIRE(s->n_kpt >= 1 && s->n_kpt <= KPN_NKPT, "n_kpt out of range: the field kernels hold 1..24 keypoints (KPN_N_KPT)");
    KPN_REQUIRE(s->sp_level >= 0 && s->sp_level <= KPN_SP_LEVEL, "sp_level out of range: the field kernels hold 0..3 octaves (KPN_SP_LEVEL)");
    return KPN_OK;
}
static bool canonical_shape(const kpn_field_shape* s) { return s->n_kpt == KPN_NKPT && s->sp_level == KPN_SP_LEVEL; }

static int check_param_table(const kpn_param_table* t) {
    KPN_REQUIRE(t && t->ani_al, "null parameter table / ani_al");
    for (int l = 0; l < P_COUNT; ++l) {
        KPN_REQUIRE(t->v_or_w[l] && t->b[l], "null weight or bias in the parameter table");
        KPN_REQUIRE((t->g[l] != nullptr) == plain_normed[l], "inconsistent parameter table: g must be set for the weight-normed layers and only for them");
    }
    return KPN_OK;
}

extern "C" size_t kpn_fold_norm_floats(void) { return 3 * (size_t)fold_norm_rows(); }

static const kpn_field_shape canonical_field_shape = {KPN_NKPT, KPN_SP_LEVEL};
extern "C" int kpn_fold_params(const kpn_param_table* table, float* plain_out, float* norms_out, void* stream) {
    return kpn_fold_params_shape(&canonical_field_shape, table, plain_out, norms_out, stream);
}
extern "C" int kpn_fold_params_backward(const kpn_param_table* table, const float* norms, const float* d_plain,
                                        const kpn_param_table* grads_table, int32_t accumulate, void* stream) {
    return kpn_fold_params_backward_shape(&canonical_field_shape, table, norms, d_plain, grads_table, accumulate, stream);
}

extern "C" int kpn_fold_params_shape(const kpn_field_shape* shape, const kpn_param_table* table, float* plain_out, float* norms_out,
                                     void* stream) {
    if (int e = check_field_shape(shape)) return e;
    if (int e = check_param_table(table)) return e;
    KPN_REQUIRE(plain_out && norms_out, "null pointer");
    KPN_REQUIRE(reinterpret_cast<uintptr_t>(norms_out) % 8 == 0, "norms_out must be 8-byte aligned");
    kpn_fold_kargs k = {};
    k.p = *table;
    fold_layers(k);
    k.plain = plain_out;
    fold_bind_norms(k, norms_out);
    k.n_kpt = shape->n_kpt; k.sp_level = shape->sp_level;
    if (canonical_shape(shape)) KPN_LAUNCH(k_fold_params<false>, dim3((unsigned)fold_rows()), dim3(64), stream, k);
    else KPN_LAUNCH(k_fold_params<true>, dim3((unsigned)fold_rows()), dim3(64), stream, k);
    return check_launch("kpn_fold_params");
}

extern "C" int kpn_fold_params_backward_shape(const kpn_field_shape* shape, const kpn_param_table* table, const float* norms,
                                              const float* d_plain, const kpn_param_table* grads_table, int32_t accumulate,
                                              void* stream) {
    if (int e = check_field_shape(shape)) return e;
    if (int e = check_param_table(table)) return e;
    KPN_REQUIRE(norms && d_plain && grads_table, "null pointer");
    KPN_REQUIRE(reinterpret_cast<uintptr_t>(norms) % 8 == 0, "norms must be 8-byte aligned");
    for (int l = 0; l < P_COUNT; ++l)
        KPN_REQUIRE(!grads_table->g[l] || plain_normed[l], "inconsistent gradient table: g set for a layer that is not weight-normed");
    kpn_fold_kargs k = {};
    k.p = *table;
    k.d = *grads_table;
    fold_layers(k);
    k.d_plain = d_plain;
    k.accumulate = accumulate != 0;
    fold_bind_norms(k, const_cast<float*>(norms));
    k.n_kpt = shape->n_kpt; k.sp_level = shape->sp_level;
    if (canonical_shape(shape)) KPN_LAUNCH(k_fold_params_backward<false>, dim3((unsigned)fold_rows()), dim3(64), stream, k);
    else KPN_LAUNCH(k_fold_params_backward<true>, dim3((unsigned)fold_rows()), dim3(64), stream, k);
    return check_launch("kpn_fold_params_backward");
}

// keypoint sets: the narrow plain vector (layers1.0's W as (128, D + 64)) <-> plain
extern "C" size_t kpn_plain_weight_floats_shape(const kpn_field_shape* shape) {
    if (check_field_shape(shape) != KPN_OK) return 0;
    const int cols = plain_dims[P_G1_0][1];
    return kpn_plain_weight_floats() - (size_t)plain_dims[P_G1_0][0] * (size_t)(cols - kpn_narrow_col(cols, shape->n_kpt, shape->sp_level));
}
extern "C" int kpn_widen_plain(const kpn_field_shape* shape, const float* narrow_dev, float* plain_dev, void* stream) {
    if (int e = check_field_shape(shape)) return e;
    KPN_REQUIRE(narrow_dev && plain_dev, "null pointer");
    const int n = (int)kpn_plain_weight_floats();
    KPN_LAUNCH(k_widen_plain, grid1d((int64_t)n, 256), dim3(256), stream, narrow_dev, plain_dev, n, plain_dims[P_G1_0][0],
               (int)shape->n_kpt, (int)shape->sp_level);
    return check_launch("kpn_widen_plain");
}
extern "C" int kpn_narrow_plain_grad(const kpn_field_shape* shape, const float* d_plain_dev, float* d_narrow_dev, int32_t accumulate,
                                     void* stream) {
    if (int e = check_field_shape(shape)) return e;
    KPN_REQUIRE(d_plain_dev && d_narrow_dev, "null pointer");
    const int n = (int)kpn_plain_weight_floats_shape(shape);
    KPN_LAUNCH(k_narrow_plain_grad, grid1d((int64_t)n, 256), dim3(256), stream, d_plain_dev, d_narrow_dev, n, plain_dims[P_G1_0][0],
               (int)shape->n_kpt, (int)shape->sp_level, (int)(accumulate != 0));
    return check_launch("kpn_narrow_plain_grad");
}

extern "C" int kpn_adam_step(const kpn_adam_args* a, void* stream) {
    KPN_REQUIRE(a && a->segments_host, "null pointer");
    KPN_REQUIRE(a->n_segments > 0, "no segments");
    KPN_REQUIRE(a->step >= 1, "step counts from 1");
    KPN_REQUIRE(a->lr >= 0.0 && a->eps >= 0.0 && a->weight_decay >= 0.0, "bad lr / eps / weight_decay");
    KPN_REQUIRE(a->beta1 >= 0.0 && a->beta1 < 1.0 && a->beta2 >= 0.0 && a->beta2 < 1.0, "betas must lie in [0, 1)");
    for (int i = 0; i < a->n_segments; ++i) {
        const kpn_adam_segment& s = a->segments_host[i];
        KPN_REQUIRE(s.param && s.grad && s.exp_avg && s.exp_avg_sq, "null pointer in an Adam segment");
        KPN_REQUIRE(s.count > 0 && s.count <= (int64_t)1 << 31, "bad Adam segment size");
    }
    // torch/optim/adam.py _single_tensor_adam: the corrections and the step size in double on the host
    const double bc1 = 1.0 - pow(a->beta1, (double)a->step), bc2 = 1.0 - pow(a->beta2, (double)a->step);
    for (int first = 0; first < a->n_segments; first += KPN_ADAM_MAX_SEGMENTS) {
        kpn_adam_kargs k = {};
        k.n_seg = std::min<int>(KPN_ADAM_MAX_SEGMENTS, a->n_segments - first);
        int64_t blocks = 0;
        for (int i = 0; i < k.n_seg; ++i) {
            k.seg[i] = a->segments_host[first + i];
            k.block0[i] = (int)blocks;
            blocks += (k.seg[i].count + 255) / 256;
            KPN_REQUIRE(blocks < (int64_t)1 << 31, "too many elements for one Adam step");
        }
        k.block0[k.n_seg] = (int)blocks;
        k.one_minus_b1 = 1.0 - a->beta1; k.b2 = a->beta2; k.one_minus_b2 = 1.0 - a->beta2;
        k.wd = a->weight_decay; k.step_size = a->lr / bc1; k.bc2_sqrt = sqrt(bc2); k.eps = a->eps;
        KPN_LAUNCH(k_adam_step, dim3((unsigned)blocks), dim3(256), stream, k);
    }
    return check_launch("kpn_adam_step");
}
