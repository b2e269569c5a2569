"""Generate the committed golden vectors in tests/golden/ by running the UNMODIFIED reference
(imported from /root/reference through oracle/ref_shim.py) on small seeded synthetic scenes.

Run in the build container only:   python -m oracle.make_golden
TEST INFRASTRUCTURE ONLY.

Each golden file holds: the complete inputs (scene tensors, hot-path state dict, cameras), and the
reference's outputs — the final out-dict of ``batch_render_pifu_nerf`` (eval, uniform=True) plus
stage-level captures obtained by wrapping the ``net`` attributes the reference itself looks up
(``net.query``, ``net.rgba2out``, ``net.importance_sample``, ``net.ray_bbox_intersection``;
reference src/model.py:979,1039,1065,1075,1085).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from keypointnerf_amd.synthetic import make_scene, perturb_reference_net  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
HOT_PREFIXES = ("mlp_geo.", "mlp_tex.", "ibr_compress_gfeat.")


def _np(t):
    return t.detach().cpu().numpy()


def scene_to_npz(scene):
    d = {"img": _np(scene["img"]), "geo0": _np(scene["feat_geo"][0]), "geo1": _np(scene["feat_geo"][1]),
         "tex": _np(scene["feat_tex"]), "fgmask": _np(scene["src_foreground_mask"]),
         "KRT": _np(scene["cam"]["KRT"]), "K": _np(scene["cam"]["K"]), "extrin": _np(scene["cam"]["extrin"]),
         "tar_K": _np(scene["cam_tar"]["K"]), "tar_RT": _np(scene["cam_tar"]["RT"]),
         "tar_meta": np.array([scene["cam_tar"]["width"], scene["cam_tar"]["height"], scene["cam_tar"]["znear"],
                               scene["cam_tar"]["zfar"]], np.float64),
         "src_meta": np.array([scene["cam"]["width"], scene["cam"]["height"], scene["cam"]["znear"],
                               scene["cam"]["zfar"], scene["cam"]["nml_scale"]], np.float64),
         "kpt3d": _np(scene["sp_data"]["kpt3d"]), "bounds": _np(scene["bounds"])}
    return {"scene." + k: v for k, v in d.items()}


class Recorder:
    """Wraps the reference's own attribute seams on ``net`` and records their inputs/outputs."""

    def __init__(self, net):
        self.net = net
        self.calls = {"query": [], "rgba2out": [], "importance_sample": [], "ray_bbox_intersection": []}
        cls = type(net)
        orig_query = net.query  # bound
        rgba2out, imp, bbox = cls.rgba2out, cls.importance_sample, cls.ray_bbox_intersection

        def q(pts, cam, *a, **k):
            out, valid = orig_query(pts, cam, *a, **k)
            self.calls["query"].append({"pts": _np(pts), "view": _np(k["view"]), "out": _np(out), "valid": _np(valid)})
            return out, valid

        def r2o(rgba, z):
            res = rgba2out(rgba, z)
            self.calls["rgba2out"].append({"rgba": _np(rgba), "z": _np(z), "color": _np(res[0]), "depth": _np(res[1]),
                                           "alpha": _np(res[2]), "contrib": _np(res[3]), "sdf": _np(res[4])})
            return res

        def im(contrib, z, n, uniform=False):
            res = imp(contrib, z, n, uniform=uniform)
            self.calls["importance_sample"].append({"contrib": _np(contrib), "z": _np(z), "out": _np(res)})
            return res

        def bb(bounds, orig, direct):
            res = bbox(bounds, orig, direct)
            self.calls["ray_bbox_intersection"].append({"bounds": _np(bounds), "orig": _np(orig), "direct": _np(direct),
                                                        "near": _np(res[0]), "far": _np(res[1]), "hit": _np(res[2])})
            return res

        net.query, net.rgba2out, net.importance_sample, net.ray_bbox_intersection = q, r2o, im, bb

    def restore(self):
        for k in ("query", "rgba2out", "importance_sample", "ray_bbox_intersection"):
            if k in self.net.__dict__:
                del self.net.__dict__[k]


def run_case(net, name, n_views, src_hw, tar_hw, mask, level, stride, Sc, Sf, seed, tar_angle=None, fine=True):
    scene = make_scene(n_views=n_views, src_hw=src_hw, tar_hw=tar_hw, mask=mask, seed=seed, tar_angle=tar_angle)
    rec = Recorder(net)
    cfg = dict(fine=fine, uniform=True, sample_per_ray_c=Sc, sample_per_ray_f=Sf,
               src_foreground_mask=scene["src_foreground_mask"], bounds=scene["bounds"])
    strd = torch.tensor([[float(stride[0]), float(stride[1])]])  # [[j, i]] as reference src/model.py:920
    with torch.no_grad():
        out = net.batch_render_pifu_nerf(net, scene["img"], scene["cam"], n_views, scene["cam_tar"], level, strd, None,
                                         scene["feat_geo"], scene["feat_tex"], dict(scene["sp_data"]), None, **cfg)
    rec.restore()
    d = scene_to_npz(scene)
    d["cfg"] = np.array([n_views, level, stride[0], stride[1], Sc, Sf], np.int64)
    for k, v in out.items():
        d["out." + k] = _np(v)
    for stage, calls in rec.calls.items():
        for i, c in enumerate(calls):
            for k, v in c.items():
                d[f"{stage}.{i}.{k}"] = v
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, **d)
    print(f"{name}: rays={out['alpha'].numel()} alpha mean={float(out['alpha_fine' if fine else 'alpha'].mean()):.4f} "
          f"valid_c={rec.calls['query'][0]['valid'].mean():.3f} -> {path} ({os.path.getsize(path)/1e6:.2f} MB)")
    return scene, out


def run_headline_case(net, name, n_views, src_hw, mask, level, stride, Sc, Sf, seed, fine=True, n_sub=2048):
    """One strided tile of a 512x512 target at the sample counts of the BASELINE configs — configs[1]: level 4 (64x64 =
    4096 rays), Sc = Sf = 64 as shipped (configs/zju.json:101-108, src/model.py:916-923); configs[4]: a 4096-ray chunk,
    V = 10, 128 flat samples (fine=False) — rendered by the reference's batch_render_pifu_nerf.  The target camera frames
    the subject like the reference's orbit (tar_focal_at_512=800, keypointnerf_amd/synthetic.py).  Source maps are kept
    at reduced resolution and the per-point stage records are subsampled (n_sub points per query call) so that the
    fixture stays small; the full out dict and the packed validity bits of every point are stored."""
    scene = make_scene(n_views=n_views, src_hw=src_hw, tar_hw=(512, 512), mask=mask, seed=seed, tar_focal_at_512=800.0)
    rec = Recorder(net)
    cfg = dict(fine=fine, uniform=True, sample_per_ray_c=Sc, sample_per_ray_f=Sf,
               src_foreground_mask=scene["src_foreground_mask"], bounds=scene["bounds"])
    strd = torch.tensor([[float(stride[0]), float(stride[1])]])
    import time
    t0 = time.time()
    with torch.no_grad():
        out = net.batch_render_pifu_nerf(net, scene["img"], scene["cam"], n_views, scene["cam_tar"], level, strd, None,
                                         scene["feat_geo"], scene["feat_tex"], dict(scene["sp_data"]), None, **cfg)
    dt = time.time() - t0
    rec.restore()
    d = scene_to_npz(scene)
    d["cfg"] = np.array([n_views, level, stride[0], stride[1], Sc, Sf], np.int64)
    d["tar_focal_at_512"] = np.float64(800.0)
    for k, v in out.items():
        d["out." + k] = _np(v)
    g = np.random.default_rng(seed)
    n_eval = 0
    for i, c in enumerate(rec.calls["query"]):
        N = c["pts"].shape[1]
        n_eval += N
        d[f"query.{i}.valid_bits"] = np.packbits(c["valid"].reshape(-1).astype(np.uint8))
        d[f"query.{i}.n"] = np.int64(N)
        idx = np.sort(g.choice(N, size=min(n_sub, N), replace=False))
        d[f"query.{i}.idx"] = idx
        for k in ("pts", "view", "out", "valid"):
            d[f"query.{i}.{k}"] = c[k][:, idx]
    for i, c in enumerate(rec.calls["rgba2out"]):                   # z of both passes for 256 rays (bin-flip diagnostics)
        d[f"rgba2out.{i}.z_sub"] = c["z"][:, ::16]
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, **d)
    key = "alpha_fine" if fine else "alpha"
    print(f"{name}: rays={out['alpha'].numel()} field evaluations={n_eval} ({dt:.1f} s of reference CPU time on "
          f"{torch.get_num_threads()} threads = {n_eval / dt:.0f} pts/s) alpha mean={float(out[key].mean()):.4f} "
          f"valid_c={rec.calls['query'][0]['valid'].mean():.3f} -> {path} ({os.path.getsize(path)/1e6:.2f} MB)")
    return n_eval, dt


def run_tiled_case(net, name, n_views, src_hw, tar_hw, mask, level, Sc, Sf, seed):
    """render_pifu_nerf's stride^2 tiles + pixel_shuffle re-assembly (reference src/model.py:897-940),
    with the image encoders bypassed (feature maps are the synthetic ones)."""
    scene = make_scene(n_views=n_views, src_hw=src_hw, tar_hw=tar_hw, mask=mask, seed=seed)
    net.attach_geo_feat = lambda im, return_val=False: scene["feat_geo"]
    net.attach_tex_feat = lambda im, return_val=False: scene["feat_tex"]
    try:
        with torch.no_grad():
            out = net.render_pifu_nerf(net, scene["img"], scene["cam"], scene["cam_tar"], level=level,
                                       sp_data=dict(scene["sp_data"]), fine=True, uniform=True, sample_per_ray_c=Sc,
                                       sample_per_ray_f=Sf, src_foreground_mask=scene["src_foreground_mask"],
                                       bounds=scene["bounds"])
    finally:
        del net.__dict__["attach_geo_feat"], net.__dict__["attach_tex_feat"]
    d = scene_to_npz(scene)
    d["cfg"] = np.array([n_views, level, 0, 0, Sc, Sf], np.int64)
    for k, v in out.items():
        d["out." + k] = _np(v)
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, **d)
    print(f"{name}: frame {tuple(out['tex_fg_fine'].shape)} -> {path} ({os.path.getsize(path)/1e6:.2f} MB)")


def run_real_encoder_case(net, name="case_s_v3_real_encoder_maps", src_hw=(128, 128), tar_hw=(32, 32), Sc=16, Sf=16, seed=31):
    """render_pifu_nerf WITH the reference's own image encoders (HGFilterV2 / ResBlkEncoder, src/utils.py:199-474, reference init
    of src/model.py:603-640) on structured source images (smooth shading + edges inside the fg masks, not white noise): the
    feature maps the field kernels see here are what the encoders actually produce — spatially smooth, O(0.1) in magnitude,
    channel-correlated — instead of the randn maps of every other fixture.  The maps the encoders returned are recorded in place
    of the synthetic ones; the frame goes through the reference tile loop at level 1."""
    scene = make_scene(n_views=3, src_hw=src_hw, tar_hw=tar_hw, mask="ellipsoid", seed=seed, tar_focal_at_512=800.0)
    H, W = src_hw
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    fg = scene["src_foreground_mask"].reshape(3, 1, H, W).float()
    base = torch.stack([0.5 + 0.4 * torch.sin(6.0 * xx + 2.0 * yy), 0.5 + 0.4 * torch.cos(5.0 * yy - xx), 0.3 + 0.5 * xx * yy], 0)
    stripes = ((torch.floor(12.0 * xx) + torch.floor(9.0 * yy)) % 2.0) * 0.25
    img = torch.stack([(base.roll(7 * v, dims=2) * (0.7 + 0.1 * v) + stripes).clamp(0, 1) for v in range(3)], 0) * fg   # fg-masked like the dataset's
    scene["img"] = img
    got = {}
    cls = type(net)

    def geo(im, return_val=False):
        r = cls.attach_geo_feat(net, im, return_val)
        got["geo"] = [x.detach().clone() for x in net.feat_geo]
        return r

    def tex(im, return_val=False):
        r = cls.attach_tex_feat(net, im, return_val)
        got["tex"] = net.feat_tex.detach().clone()
        return r

    net.attach_geo_feat, net.attach_tex_feat = geo, tex
    try:
        with torch.no_grad():
            out = net.render_pifu_nerf(net, scene["img"], scene["cam"], scene["cam_tar"], level=1, sp_data=dict(scene["sp_data"]),
                                       fine=True, uniform=True, sample_per_ray_c=Sc, sample_per_ray_f=Sf,
                                       src_foreground_mask=scene["src_foreground_mask"], bounds=scene["bounds"])
    finally:
        del net.__dict__["attach_geo_feat"], net.__dict__["attach_tex_feat"]
    scene["feat_geo"], scene["feat_tex"] = got["geo"], got["tex"]
    d = scene_to_npz(scene)
    d["cfg"] = np.array([3, 1, 0, 0, Sc, Sf], np.int64)
    d["tar_focal_at_512"] = np.float64(800.0)
    for k, v in out.items():
        d["out." + k] = _np(v)
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, **d)
    st = lambda t: f"|max| {float(t.abs().max()):.3f} std {float(t.std()):.3f}"
    print(f"{name}: frame {tuple(out['tex_fg_fine'].shape)} alpha mean {float(out['alpha_fine'].mean()):.3f}; encoder maps: geo0 {tuple(got['geo'][0].shape)} "
          f"{st(got['geo'][0])}, geo1 {tuple(got['geo'][1].shape)} {st(got['geo'][1])}, tex {tuple(got['tex'].shape)} {st(got['tex'])} -> {path} "
          f"({os.path.getsize(path)/1e6:.2f} MB)")


def run_train_case(net, name, n_views, src_hw, tar_hw, mask, Sc, Sf, seed, patch=12, noise_std=0.01):
    """TRAIN branch of batch_render_pifu_nerf (reference src/model.py:1008-1017,1049-1053,993-994,742-748,1129)
    with every random draw recorded: torch.rand_like / randn_like / rand are wrapped for the duration of the call,
    np.random.randint is seeded.  The view-dropout keep vectors are rebuilt from the recorded draws with the
    reference's own formula (:743-747)."""
    scene = make_scene(n_views=n_views, src_hw=src_hw, tar_hw=tar_hw, mask=mask, seed=seed)
    Ht, Wt = tar_hw
    g = torch.Generator().manual_seed(seed)
    # target-view foreground mask `msk` (decode_batch passes images_masks[:,0], src/model.py:312,391): a disc
    yy, xx = torch.meshgrid(torch.arange(Ht), torch.arange(Wt), indexing="ij")
    msk = (((yy - Ht / 2) ** 2 + (xx - Wt / 2) ** 2) < (0.3 * min(Ht, Wt)) ** 2)[None, None]
    log = []
    orig = {"rand_like": torch.rand_like, "randn_like": torch.randn_like, "rand": torch.rand}

    def wrap(nm):
        def f(*a, **k):
            r = orig[nm](*a, **k)
            log.append((nm, r.clone()))
            return r
        return f

    net.train()
    net.train_out_h = net.train_out_w = patch
    rec = Recorder(net)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.rand_like, torch.randn_like, torch.rand = wrap("rand_like"), wrap("randn_like"), wrap("rand")
    try:
        cfg = dict(fine=True, uniform=False, sample_per_ray_c=Sc, sample_per_ray_f=Sf, rand_noise_std=noise_std,
                   src_foreground_mask=scene["src_foreground_mask"], bounds=scene["bounds"], msk=msk)
        with torch.no_grad():
            out = net.batch_render_pifu_nerf(net, scene["img"], scene["cam"], n_views, scene["cam_tar"], 5, 0, None,
                                             scene["feat_geo"], scene["feat_tex"], dict(scene["sp_data"]), None, **cfg)
    finally:
        torch.rand_like, torch.randn_like, torch.rand = orig["rand_like"], orig["randn_like"], orig["rand"]
        rec.restore()
        net.eval()
    # draws in call order: rand_like(z) | query coarse: rand_like(dropout[:,1:]), rand_like(dropout) | randn_like(rad)
    #                      | rand (importance u) | query fine: rand_like x2 | randn_like(rad)
    names = [n for n, _ in log]
    assert names == ["rand_like", "rand_like", "rand_like", "randn_like", "rand", "rand_like", "rand_like", "randn_like"], names
    t = [x for _, x in log]

    def keep_vec(r_mask, r_perm):                                  # src/model.py:743-747
        d = torch.zeros(1, n_views, 1, 1)
        d[:, :1] = 1.0
        d[:, 1:] = (r_mask > 0.5).float()
        return torch.gather(d, 1, r_perm.argsort(dim=1)).reshape(-1)

    keep_c, keep_f = keep_vec(t[1], t[2]), keep_vec(t[5], t[6])
    # the patch pixels (src/model.py:1010-1016), np.random.randint replayed with the same seed
    np.random.seed(seed)
    coords = torch.stack(torch.where(msk.squeeze())[::-1], -1)
    center = coords[np.random.randint(0, coords.shape[0], 1)]
    yg, xg = torch.meshgrid(torch.arange(0, patch), torch.arange(0, patch), indexing="ij")
    grids = torch.stack([xg, yg], -1).view(-1, 2) + (center - patch // 2)
    grids = grids.clamp(0, min(Wt - 1, Ht - 1))
    d = scene_to_npz(scene)
    d.update({"cfg": np.array([n_views, 5, 0, 0, Sc, Sf], np.int64), "pix": _np(grids).astype(np.int32),
              "u_c": _np(t[0])[0], "noise_c": _np(t[3]).reshape(-1), "u_f": _np(t[4])[0], "noise_f": _np(t[7]).reshape(-1),
              "keep_c": _np(keep_c), "keep_f": _np(keep_f), "noise_std": np.float32(noise_std), "msk": _np(msk)})
    for k, v in out.items():
        d["out." + k] = _np(v)
    d["dirs"] = rec.calls["ray_bbox_intersection"][0]["direct"][0]
    d["z_c"] = rec.calls["rgba2out"][0]["z"][0]
    d["z_f"] = rec.calls["rgba2out"][1]["z"][0]
    d["valid_c"] = rec.calls["query"][0]["valid"].reshape(-1)
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, **d)
    print(f"{name}: rays={grids.shape[0]} keep_c={keep_c.tolist()} keep_f={keep_f.tolist()} alpha_fine={float(out['alpha_fine'].mean()):.3f} "
          f"valid_c={d['valid_c'].mean():.3f} -> {path} ({os.path.getsize(path)/1e6:.2f} MB)")


def run_rgba2out_grad_case(name, seed=11, R=40, S=24):
    """Gradients of the reference's rgba2out by torch autograd (first piece of the training backward)."""
    rmodel = ref_shim.load_reference()
    g = torch.Generator().manual_seed(seed)
    rgba = torch.rand(1, R, S, 5, generator=g)
    rgba[..., 0] = torch.relu(torch.randn(1, R, S, generator=g)) * 6.0          # sigma >= 0, many exact zeros
    rgba[..., 1] = torch.randn(1, R, S, generator=g) * 0.01
    rgba[0, :4, :, 0] = 0.0                                                    # rays with no density at all
    z = (torch.rand(1, R, S, generator=g) * 0.2 + 0.01).cumsum(-1) + 2.0
    rgba.requires_grad_(True)
    color, depth, alpha, contrib, sdf = rmodel.KeypointNeRF.rgba2out(rgba, z)
    d_color, d_depth = torch.randn(color.shape, generator=g), torch.randn(depth.shape, generator=g)
    d_alpha, d_sdf = torch.randn(alpha.shape, generator=g), torch.randn(sdf.shape, generator=g)
    (g_all,) = torch.autograd.grad([color, depth, alpha, sdf], [rgba], [d_color, d_depth, d_alpha, d_sdf], retain_graph=True)
    (g_col,) = torch.autograd.grad([color], [rgba], [d_color])
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, rgba=_np(rgba), z=_np(z), d_color=_np(d_color), d_depth=_np(d_depth), d_alpha=_np(d_alpha),
                        d_sdf=_np(d_sdf), g_all=_np(g_all), g_color_only=_np(g_col))
    print(f"{name}: |g|max={float(g_all.abs().max()):.3g} -> {path}")


def run_geo_rows_grad_case(net, name, n_views, src_hw, mask, n_pts, seed, S=8):
    """Gradients of the per-(point,view) geometry rows by the reference's own autograd: a forward hook on
    net.mlp_geo.layers1 (MLPUNet, src/utils.py:691-720) captures x_view inside an unmodified net.query() call;
    loss = sum(x_view * G) with G zeroed on masked points (their pooling weights are 0, so no gradient reaches
    them in training).  Recorded: d loss / d (effective weight, bias, weight_g, weight_v) of layers1 and
    d loss / d feat_geo[0], feat_geo[1]."""
    scene = make_scene(n_views=n_views, src_hw=src_hw, tar_hw=(16, 16), mask=mask, seed=seed)
    g = torch.Generator().manual_seed(seed)
    lo, hi = scene["bounds"].reshape(2, 3)[0], scene["bounds"].reshape(2, 3)[1]
    pts = (lo + (hi - lo) * torch.rand(n_pts, 3, generator=g))[None]
    view = torch.nn.functional.normalize(torch.randn(n_pts, 3, generator=g), dim=-1)[None]
    feat_geo = [f.clone().requires_grad_(True) for f in scene["feat_geo"]]
    captured, eff = {}, {}
    l1 = net.mlp_geo.layers1
    hooks = [l1.register_forward_hook(lambda m, i, o: captured.__setitem__("x_view", o))]
    for li, layer in enumerate(l1.layers):
        def fh(m, i, o, li=li):
            m.weight.retain_grad()
            eff[li] = m.weight
        hooks.append(layer.linear.register_forward_hook(fh))
    net.eval()
    out, valid = net.query(pts, scene["cam"], feat_geo, scene["feat_tex"], n_views=n_views, view=view, nerf=True,
                           sp_data=dict(scene["sp_data"]), tx_data={"img": scene["img"]}, bbox_center=None, n_pts_samples=S,
                           src_foreground_mask=scene["src_foreground_mask"])
    for h in hooks:
        h.remove()
    x_view = captured["x_view"]                                           # (B, V, N, 64)
    assert x_view.shape == (1, n_views, n_pts, 64), x_view.shape
    G = torch.randn(x_view.shape, generator=g) * valid.reshape(1, 1, n_pts, 1).float()
    params = dict(l1.named_parameters())
    net.zero_grad()
    (x_view * G).sum().backward()
    d = scene_to_npz(scene)
    d.update({"cfg": np.array([n_views, 0, 0, 0, 0, 0], np.int64), "pts": _np(pts[0]), "view": _np(view[0]), "valid": _np(valid).reshape(-1), "x_view": _np(x_view[0]),
              "G": _np(G[0].permute(1, 0, 2)),                             # (N, V, 64), the C-ABI layout
              "d_geo0": _np(feat_geo[0].grad), "d_geo1": _np(feat_geo[1].grad)})
    for li in range(4):
        d[f"dW{li}"] = _np(eff[li].grad)
        d[f"db{li}"] = _np(params[f"layers.{li}.linear.bias"].grad)
    for k, v in params.items():
        d["param_grad." + k] = _np(v.grad)
    net.zero_grad()
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, **d)
    print(f"{name}: N={n_pts} valid={float(valid.float().mean()):.3f} |dW0|max={float(eff[0].grad.abs().max()):.3g} "
          f"|d_geo0|max={float(feat_geo[0].grad.abs().max()):.3g} -> {path} ({os.path.getsize(path)/1e6:.2f} MB)")


def run_query_grad_case(net, name, n_views, src_hw, mask, n_pts, seed, S=8, keep=None):
    """Gradients of the WHOLE field evaluation by the reference's own autograd: an unmodified net.query() call in
    eval mode (no random dropout), loss = sum(out * G) with (a) out = query's raw [sdf_raw, rad, rgb] and
    (b) out = eval_func(query) restated from src/model.py:981-996 (mask*relu(rad), mask*sdf + (1-mask)*0.1/nml_scale).
    Recorded per variant: d loss / d every hot-path parameter (effective weights via retain_grad on the
    weight-normed tensors, plus the raw weight_g / weight_v / bias / ani_al grads) and d loss / d feat_geo[0],
    feat_geo[1], feat_tex."""
    from keypointnerf_amd.synthetic import HOTPATH_LAYERS
    scene = make_scene(n_views=n_views, src_hw=src_hw, tar_hw=(16, 16), mask=mask, seed=seed)
    g = torch.Generator().manual_seed(seed)
    lo, hi = scene["bounds"].reshape(2, 3)[0], scene["bounds"].reshape(2, 3)[1]
    pts = (lo + (hi - lo) * torch.rand(n_pts, 3, generator=g))[None]
    view = torch.nn.functional.normalize(torch.randn(n_pts, 3, generator=g), dim=-1)[None]
    G = torch.randn(1, n_pts, 5, generator=g)
    d = scene_to_npz(scene)
    d.update({"cfg": np.array([n_views, 0, 0, 0, 0, 0], np.int64), "pts": _np(pts[0]), "view": _np(view[0]), "G": _np(G[0])})
    net.eval()
    for variant in ("raw", "evalfunc"):
        feat_geo = [f.clone().requires_grad_(True) for f in scene["feat_geo"]]
        feat_tex = scene["feat_tex"].clone().requires_grad_(True)
        eff, hooks = {}, []
        for lname, prefix, shape, wn in HOTPATH_LAYERS:
            mod = net.get_submodule(prefix)
            def fh(m, i, o, lname=lname):
                if not m.weight.is_leaf:
                    m.weight.retain_grad()
                eff[lname] = m.weight
            hooks.append(mod.register_forward_hook(fh))
        net.zero_grad()
        out, valid = net.query(pts, scene["cam"], feat_geo, feat_tex, n_views=n_views, view=view, nerf=True,
                               sp_data=dict(scene["sp_data"]), tx_data={"img": scene["img"]}, bbox_center=None, n_pts_samples=S,
                               src_foreground_mask=scene["src_foreground_mask"])
        for h in hooks:
            h.remove()
        if variant == "evalfunc":                                           # src/model.py:981-996, rand_noise_std = 0
            m = valid.float()
            sdf = m * out[..., :1] + (1.0 - m) * (0.1 / scene["cam"]["nml_scale"])
            sigma = m * torch.relu(out[..., 1:2])
            res = torch.cat([sigma, sdf, out[..., 2:]], -1)
        else:
            res = out
        (res * G).sum().backward()
        pre = variant + "."
        d[pre + "out"], d[pre + "valid"] = _np(res[0]), _np(valid).reshape(-1)
        d[pre + "d_geo0"], d[pre + "d_geo1"], d[pre + "d_tex"] = _np(feat_geo[0].grad), _np(feat_geo[1].grad), _np(feat_tex.grad)
        for lname, prefix, shape, wn in HOTPATH_LAYERS:
            mod = net.get_submodule(prefix)
            d[pre + "dW." + lname] = _np(eff[lname].grad)
            d[pre + "db." + lname] = _np(mod.bias.grad)
        d[pre + "d_ani_al"] = _np(net.mlp_tex.ani_al.grad).reshape(1)
        for k, v in net.named_parameters():
            if k.startswith(HOT_PREFIXES) and v.grad is not None:
                d[pre + "param_grad." + k] = _np(v.grad)
        print(f"{name}/{variant}: N={n_pts} valid={float(valid.float().mean()):.3f} |d_tex|max={float(feat_tex.grad.abs().max()):.3g} "
              f"d_ani={float(net.mlp_tex.ani_al.grad):.4g}")
    net.zero_grad()
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, **d)
    print(f"{name} -> {path} ({os.path.getsize(path)/1e6:.2f} MB)")


def run_train_grad_case(net, name, n_views, src_hw, tar_hw, mask, Sc, Sf, seed, patch=8, noise_std=0.01):
    """loss.backward() through the TRAIN branch of batch_render_pifu_nerf (the field part of training_step,
    src/model.py:128-155): the unmodified reference in train mode, every random draw recorded as in run_train_case,
    loss = sum_k <out_k, G_k> over its seven outputs.  Recorded: the gradients of every hot-path parameter
    (weight_g / weight_v / weight / bias / ani_al) and of feat_geo[0], feat_geo[1], feat_tex."""
    scene = make_scene(n_views=n_views, src_hw=src_hw, tar_hw=tar_hw, mask=mask, seed=seed)
    Ht, Wt = tar_hw
    yy, xx = torch.meshgrid(torch.arange(Ht), torch.arange(Wt), indexing="ij")
    msk = (((yy - Ht / 2) ** 2 + (xx - Wt / 2) ** 2) < (0.3 * min(Ht, Wt)) ** 2)[None, None]
    log = []
    orig = {"rand_like": torch.rand_like, "randn_like": torch.randn_like, "rand": torch.rand}

    def wrap(nm):
        def f(*a, **k):
            r = orig[nm](*a, **k)
            log.append((nm, r.clone()))
            return r
        return f

    feat_geo = [f.clone().requires_grad_(True) for f in scene["feat_geo"]]
    feat_tex = scene["feat_tex"].clone().requires_grad_(True)
    net.train()
    net.train_out_h = net.train_out_w = patch
    rec = Recorder(net)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.rand_like, torch.randn_like, torch.rand = wrap("rand_like"), wrap("randn_like"), wrap("rand")
    try:
        cfg = dict(fine=True, uniform=False, sample_per_ray_c=Sc, sample_per_ray_f=Sf, rand_noise_std=noise_std,
                   src_foreground_mask=scene["src_foreground_mask"], bounds=scene["bounds"], msk=msk)
        net.zero_grad()
        out = net.batch_render_pifu_nerf(net, scene["img"], scene["cam"], n_views, scene["cam_tar"], 5, 0, None,
                                         feat_geo, feat_tex, dict(scene["sp_data"]), None, **cfg)
        gen = torch.Generator().manual_seed(seed + 100)
        keys = ["tex_fg", "depth", "alpha", "tex_fg_fine", "depth_fine", "alpha_fine", "sdf"]
        G = {k: torch.randn(out[k].shape, generator=gen) for k in keys}
        sum((out[k] * G[k]).sum() for k in keys).backward()
    finally:
        torch.rand_like, torch.randn_like, torch.rand = orig["rand_like"], orig["randn_like"], orig["rand"]
        rec.restore()
        net.eval()
    names = [n for n, _ in log]
    assert names == ["rand_like", "rand_like", "rand_like", "randn_like", "rand", "rand_like", "rand_like", "randn_like"], names
    t = [x for _, x in log]

    def keep_vec(r_mask, r_perm):                                  # src/model.py:743-747
        dd = torch.zeros(1, n_views, 1, 1)
        dd[:, :1] = 1.0
        dd[:, 1:] = (r_mask > 0.5).float()
        return torch.gather(dd, 1, r_perm.argsort(dim=1)).reshape(-1)

    keep_c, keep_f = keep_vec(t[1], t[2]), keep_vec(t[5], t[6])
    np.random.seed(seed)
    coords = torch.stack(torch.where(msk.squeeze())[::-1], -1)
    center = coords[np.random.randint(0, coords.shape[0], 1)]
    yg, xg = torch.meshgrid(torch.arange(0, patch), torch.arange(0, patch), indexing="ij")
    grids = torch.stack([xg, yg], -1).view(-1, 2) + (center - patch // 2)
    grids = grids.clamp(0, min(Wt - 1, Ht - 1))
    d = scene_to_npz(scene)
    d.update({"cfg": np.array([n_views, 5, 0, 0, Sc, Sf], np.int64), "pix": _np(grids).astype(np.int32),
              "u_c": _np(t[0])[0], "noise_c": _np(t[3]).reshape(-1), "u_f": _np(t[4])[0], "noise_f": _np(t[7]).reshape(-1),
              "keep_c": _np(keep_c), "keep_f": _np(keep_f), "noise_std": np.float32(noise_std)})
    for k in keys:
        d["out." + k] = _np(out[k])
        d["G." + k] = _np(G[k])
    d["d_geo0"], d["d_geo1"], d["d_tex"] = _np(feat_geo[0].grad), _np(feat_geo[1].grad), _np(feat_tex.grad)
    for k, v in net.named_parameters():
        if k.startswith(HOT_PREFIXES) and v.grad is not None:
            d["param_grad." + k] = _np(v.grad)
    net.zero_grad()
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, **d)
    print(f"{name}: rays={grids.shape[0]} keep_c={keep_c.tolist()} keep_f={keep_f.tolist()} alpha_fine={float(out['alpha_fine'].mean()):.3f} "
          f"|d_tex|max={float(feat_tex.grad.abs().max()):.3g} -> {path} ({os.path.getsize(path)/1e6:.2f} MB)")


def run_output_case(name, seed=9):
    """Output side: the reference's own frame arrangement / quantisation / PSNR."""
    rmodel = ref_shim.load_reference()
    import src.zju_evaluator as rzju
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(1, 3, 24, 20, generator=g) * 1.3 - 0.15          # values outside [0,1] exercise the clamp
    gt = torch.rand(1, 3, 24, 20, generator=g)
    hwc = rmodel.KeypointNeRFLightningModule._arrange_nerf_images({"tex_fg_fine": pred}, 2.0, 8.0)  # model.py:427-430
    rgb8 = (hwc * 255.).astype(np.uint8)                                                              # model.py:496
    a = pred.clamp(0, 1).squeeze(0).permute(1, 2, 0).numpy()
    b = gt.squeeze(0).permute(1, 2, 0).numpy()
    mse = float(np.mean((a - b) ** 2))                                                                # zju_evaluator.py:63
    psnr = float(rzju.ZJUEvaluator._compute_psnr(a, b))                                               # :16-19
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, pred=_np(pred), gt=_np(gt), hwc=hwc, rgb8=rgb8, bgr8=rgb8[:, :, ::-1].copy(),
                        mse=np.float64(mse), psnr=np.float64(psnr))
    print(f"{name}: psnr={psnr:.4f} -> {path}")


def run_loss_case(name="case_r_loss", seed=23):
    """The reference's training loss (compute_error, src/utils.py:97-171) with the shipped lambdas (configs/zju.json:
    109-119) on a random 64x64 patch as KeypointNeRF.forward assembles it (src/model.py:885-894; VGG stubbed out: it needs
    downloaded weights), and the gradients loss.backward() sends to tex_fg / tex_fg_fine."""
    rmodel = ref_shim.load_reference()
    import src.utils as rutils
    cfg = ref_shim.load_config()

    def find(d, key):
        if isinstance(d, dict):
            if key in d:
                return d[key]
            for v in d.values():
                r = find(v, key)
                if r is not None:
                    return r
        return None
    lambdas = find(cfg, "lambdas")
    g = torch.Generator().manual_seed(seed)
    tex_c = torch.rand(1, 3, 64, 64, generator=g).requires_grad_(True)
    tex_f = torch.rand(1, 3, 64, 64, generator=g).requires_grad_(True)
    tar = torch.rand(1, 3, 64, 64, generator=g)
    with torch.no_grad():
        tar[0, :, :8] = tex_f[0, :, :8]          # exact ties: abs'(0) = 0 in torch
    out = {"tex_fg": tex_c, "tex_fg_fine": tex_f, "tar_img": tar, "tex": tex_c, "tex_cal": tex_c, "tex_fine": tex_f,
           "tex_cal_fine": tex_f}
    loss, err = rutils.compute_error(out_nerf=out, vggloss=None, lambdas=lambdas)
    loss.backward()
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, tex_fg=_np(tex_c), tex_fg_fine=_np(tex_f), tar_img=_np(tar), loss=np.float32(float(loss)),
                        e_pix_c=np.float32(float(err["e_pix_c"])), e_pix_l1=np.float32(float(err["e_pix_l1"])),
                        err_keys=np.array(sorted(err.keys())), d_tex_fg=_np(tex_c.grad), d_tex_fg_fine=_np(tex_f.grad),
                        lambda_l1_c=np.float32(lambdas["lambda_l1_c"]), lambda_l1=np.float32(lambdas["lambda_l1"]),
                        lambdas_json=np.array(__import__("json").dumps(lambdas)))
    print(f"{name}: loss={float(loss):.6f} keys={sorted(err.keys())} -> {path}")


def run_loss_lambdas_case(name="case_u_loss_lambdas", seed=3):
    """The reference's compute_error (src/utils.py:97-171) beyond the shipped lambdas: l2 / lp / mask loss switched on, an ssim
    weight and `*top*` keys present (both without effect in the reference), weights of 0 — its keys, values and total per lambda set."""
    ref_shim.load_reference()
    import src.utils as rutils
    g = torch.Generator().manual_seed(seed)
    out = {"tex_cal": torch.rand(1, 3, 8, 8, generator=g), "tex_cal_fine": torch.rand(1, 3, 8, 8, generator=g),
           "alpha": torch.rand(1, 1, 8, 8, generator=g), "alpha_fine": torch.rand(1, 1, 8, 8, generator=g),
           "tar_img": torch.rand(1, 3, 8, 8, generator=g), "tar_alpha": (torch.rand(1, 1, 8, 8, generator=g) > 0.5).float()}
    sets = ({"lambda_l1": 10.0, "lambda_l1_c": 1.0, "lambda_vgg": 0.5},
            {"lambda_l1": 2.0, "lambda_l1_c": 0.0, "lambda_l2": 3.0, "lambda_lp": 0.5, "lambda_ssim": 1.0, "lambda_mloss": 4.0,
             "lambda_l1top30": 1.0, "lambda_l2top10": 0.0})
    d = {"in." + k: _np(v) for k, v in out.items()}
    d["n_sets"] = np.int32(len(sets))
    for i, lambdas in enumerate(sets):
        loss, err = rutils.compute_error(out, None, lambdas)
        keys = sorted(err)
        d[f"set{i}.lambdas_json"] = np.array(__import__("json").dumps(lambdas))
        d[f"set{i}.keys"] = np.array(keys)
        d[f"set{i}.values"] = np.array([float(err[k]) for k in keys], np.float64)
        d[f"set{i}.loss"] = np.float64(float(loss))
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, **d)
    print(f"{name}: {len(sets)} lambda sets -> {path}")


def main():
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    net = ref_shim.build_reference_net(seed=0)
    perturb_reference_net(net, seed=7)
    if "--only-nofgmask" in sys.argv:  # add case M without rewriting the other (unchanged) files
        run_nofgmask_case(net)
        return
    if "--only-sigma" in sys.argv:
        run_sigma_nofine_case(net)
        return
    if "--only-loss" in sys.argv:
        run_loss_case()
        return
    if "--only-loss-lambdas" in sys.argv:
        run_loss_lambdas_case()
        return
    if "--only-headline" in sys.argv:
        run_headline_cases(net)
        return
    if "--only-real-encoders" in sys.argv:
        run_real_encoder_case(net)
        return
    sd = {k: _np(v) for k, v in net.state_dict().items() if k.startswith(HOT_PREFIXES)}
    np.savez_compressed(os.path.join(GOLDEN_DIR, "weights_ref_seed0.npz"), **sd)
    print("weights:", sum(v.size for v in sd.values()), "floats")
    # A: shipped view count, ellipsoid mask, level 1 (every pixel of a 32x32 target)
    run_case(net, "case_a_v3_ellipsoid", 3, (64, 64), (32, 32), "ellipsoid", 1, (0, 0), 16, 16, seed=1)
    # B: V=4, dense mask, non-square source and target, level 2 tile with offset (j=1,i=0), Sc != Sf (the reference needs (Sc+Sf) % Sf == 0, src/model.py:808,835)
    run_case(net, "case_b_v4_dense_tile", 4, (48, 80), (32, 48), "dense", 2, (1, 0), 24, 12, seed=2)
    # C: a target camera far off the ring so that many rays miss the AABB / leave the source frusta
    run_case(net, "case_c_v3_offaxis", 3, (64, 64), (24, 24), "dense", 1, (0, 0), 8, 8, seed=3, tar_angle=95.0)
    # D: full-frame assembly through the reference tile loop + pixel_shuffle
    run_tiled_case(net, "case_d_v3_tiled_frame", 3, (64, 64), (16, 16), "ellipsoid", 3, 8, 8, seed=4)
    run_output_case("case_e_output")
    run_rgba2out_grad_case("case_h_rgba2out_grad")
    # F/G: train branch with recorded random draws (seeds chosen so that at least one view is dropped in one of them)
    run_train_case(net, "case_f_v3_train", 3, (64, 64), (32, 32), "dense", 12, 12, seed=5)
    run_train_case(net, "case_g_v4_train", 4, (48, 80), (32, 48), "ellipsoid", 16, 8, seed=8)
    run_geo_rows_grad_case(net, "case_i_v3_geo_rows_grad", 3, (64, 64), "ellipsoid", 600, seed=12)
    run_query_grad_case(net, "case_j_v3_query_grad", 3, (64, 64), "ellipsoid", 400, seed=13)
    # seeds chosen for informative dropout patterns: k = coarse all views / fine drops view 1; l = nothing dropped
    run_train_grad_case(net, "case_k_v3_train_grad", 3, (64, 64), (32, 32), "ellipsoid", 12, 12, seed=6)
    run_train_grad_case(net, "case_l_v3_train_grad", 3, (64, 64), (32, 32), "ellipsoid", 12, 12, seed=10)
    run_nofgmask_case(net)
    run_sigma_nofine_case(net)
    run_headline_cases(net)
    run_loss_case()
    run_loss_lambdas_case()
    run_real_encoder_case(net)


def run_headline_cases(net):
    # P: BASELINE configs[1] — one level-4 strided tile (offset j=3, i=5) of a 512^2 target, V=3, 64 + 64 samples
    run_headline_case(net, "case_p_v3_headline_tile", 3, (128, 128), "ellipsoid", 4, (3, 5), 64, 64, seed=21)
    # Q: BASELINE configs[4] — one 4096-ray chunk, V=10, 128 flat samples, dense mask
    run_headline_case(net, "case_q_v10_flat128_chunk", 10, (96, 96), "dense", 4, (6, 2), 128, 128, seed=22, fine=False)


def run_sigma_nofine_case(net):
    # N: a different keypoint-weight width (sp_args['sigma'], src/spatial.py:112-114) and fine=False (src/model.py:1067:
    # no importance samples, no fine keys in the out dict)
    old = net.sp_encoder.kwargs.get("sigma")
    net.sp_encoder.kwargs["sigma"] = 0.25
    try:
        run_case(net, "case_n_v3_sigma_nofine", 3, (64, 64), (24, 24), "ellipsoid", 1, (0, 0), 12, 8, seed=15, fine=False)
    finally:
        net.sp_encoder.kwargs["sigma"] = old


def run_nofgmask_case(net):
    # M: model_cfg['disable_fg_mask'] = True (src/model.py:566, 734-735) on a scene whose fg masks are NOT all ones: the
    # masks must be ignored, only the frustum test decides validity
    net.disable_fg_mask = True
    try:
        run_case(net, "case_m_v3_nofgmask", 3, (64, 64), (24, 24), "ellipsoid", 1, (0, 0), 8, 8, seed=14)
    finally:
        net.disable_fg_mask = False


if __name__ == "__main__":
    main()
