"""Records tests/golden/case_w_encoders.npz from the live, unmodified reference classes HGFilterV2 and ResBlkEncoder
(src/utils.py:199-474, loaded through oracle/ref_shim) built with the shipped arguments (configs/zju.json:46-51,82-89):

    python scripts/make_encoder_golden.py

Parameters: the reference's own init_weights (src/model.py:610-640), then tests/encoder_golden.perturb on every parameter; the
file keeps the seeds and a checksum per parameter tensor (the tests rebuild the weights).  It also asserts that the stand-in
modules of tests/encoder_golden.py have bit-identical parameters and give bit-identical fp32 outputs on the CPU for every
small case, which pins them to the reference.  Recorded per small case: the seed of the source images (tests/encoder_golden.case_image), ds, the reference's outputs with
the module in fp64 (full for the first case, with its fp32 outputs and the reference's e_ref of every named stage, whose hooked tensors must equal the
stand-in's bit for bit; a seeded sample of positions for the others, indices stored, to keep the file small) and e_ref = max|fp32 - fp64| per output; for the shipped size (3, 3, 512, 512) the fp64 values and e_ref on a seeded
sample of positions per map.  Arrays, seeds and names only.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402
from tests import encoder_golden as eg  # noqa: E402

SEED_GEO, SEED_TEX, N_SAMPLE = 20261, 20262, 2048
CASES = {"a": ((1, 3, 128, 128), 1), "b": ((2, 3, 128, 256), 1), "c": ((1, 3, 256, 128), 1), "odd": ((1, 3, 50, 38), 0),
         "full": ((3, 3, 512, 512), 1)}


def main():
    model = ref_shim.load_reference()
    utils = sys.modules[model.HGFilterV2.__module__] if hasattr(model, "HGFilterV2") else None
    HG = getattr(model, "HGFilterV2", None) or utils.HGFilterV2
    RB = getattr(model, "ResBlkEncoder", None) or utils.ResBlkEncoder
    init = model.KeypointNeRF.init_weights
    ref_geo, ref_tex = HG(**eg.GEO_ARGS), RB(**eg.TEX_ARGS)
    out = {"seed_geo": SEED_GEO, "seed_tex": SEED_TEX}
    nets = {}
    for tag, ref, seed, mk in (("geo", ref_geo, SEED_GEO, eg.stand_in_geo), ("tex", ref_tex, SEED_TEX, eg.stand_in_tex)):
        init(ref)
        eg.perturb(ref, seed)
        ref.eval()
        mine = mk(seed)
        rp = [(n, p) for n, p in ref.named_parameters()]
        mp = dict(mine.named_parameters())
        assert len(rp) == len(mp), (tag, len(rp), len(mp))
        for n, p in rp:
            assert torch.equal(p, mp[n]), (tag, n)
        assert [n for n, _ in rp] == list(mp), "parameter order"
        out[f"checksum_{tag}"] = eg.checksums(ref)
        nets[tag] = (ref, mine)
    for ci, (name, (shape, ds)) in enumerate(CASES.items()):
        img = eg.case_image(shape, 77 + ci)
        x = eg.net_input(img, ds)
        rng = np.random.default_rng(5)
        out[f"{name}_img_shape"], out[f"{name}_img_seed"], out[f"{name}_ds"] = np.array(shape), 77 + ci, ds
        for tag in ("geo", "tex"):
            if tag == "geo" and name == "odd":
                continue
            ref, mine = nets[tag]
            with torch.no_grad():
                r32 = ref(x)
                if name != "full":
                    m32 = mine(x)
                ref.double()
                r64 = ref(x.double())
                ref.float()
            r32, r64 = (r32 if tag == "geo" else [r32]), (r64 if tag == "geo" else [r64])
            if name == "a":
                # the named stage tensors: hooked on the live reference and on the stand-in, bit for bit; e_ref per stage
                names = {n: n for n in eg.GEO_STAGE_MODULES} if tag == "geo" else eg.TEX_STAGE_MODULES
                _, sr = eg.run_with_stages(ref, x, names)
                _, sm = eg.run_with_stages(mine, x, names)
                ref.double()
                _, sr64 = eg.run_with_stages(ref, x.double(), names)
                ref.float()
                for k in names:
                    assert torch.equal(sr[k], sm[k]), f"stage {k} of the stand-in differs from the reference ({tag})"
                    out[f"a_{tag}_stage_eref_{k}"] = float((sr[k].double() - sr64[k]).abs().max())
                for i, a in enumerate(r32):
                    out[f"a_{tag}{i}_f32"] = a.numpy()
            if name != "full":
                m32 = m32 if tag == "geo" else [m32]
                for a, b in zip(r32, m32):
                    assert torch.equal(a, b), f"stand-in differs from the reference: {tag} case {name}"
            for i, (a, b) in enumerate(zip(r32, r64)):
                key = f"{name}_{tag}{i}"
                out[key + "_eref"] = float((a.double() - b).abs().max())
                out[key + "_shape"] = np.array(b.shape)
                flat = b.reshape(-1).numpy()
                if name == "a" or flat.size <= N_SAMPLE:
                    out[key + "_f64"] = b.numpy()
                else:
                    idx = np.sort(rng.choice(flat.size, N_SAMPLE, replace=False))
                    out[key + "_idx"], out[key + "_f64"] = idx.astype(np.int64), flat[idx]
                print(key, tuple(b.shape), "e_ref", out[key + "_eref"], "max", float(b.abs().max()), flush=True)
    np.savez_compressed(eg.GOLDEN, **out)
    print("wrote", eg.GOLDEN, os.path.getsize(eg.GOLDEN))


if __name__ == "__main__":
    main()
