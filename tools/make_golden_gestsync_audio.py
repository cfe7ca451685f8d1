"""Generate tests/golden/gestsync_audio.npz by running the REAL reference's GestSync.forward_aud (build container only, like
oracle/make_golden.py, whose reference import and strict loader it uses; never runs on the GPU box).

    python tools/make_golden_gestsync_audio.py

Weights: the seeded synthetic `gauss` state dict (jegal_amd.synth), loaded with strict=True.  Inputs: np.random.default_rng(seed)
.standard_normal((29, 1, 80, 100)) float32 -- only the seed is stored, tests regenerate them.  Stored: seed, the (29, 1024) output of
forward_aud and the fraction of active units behind every ReLU (a replay of the layers, checked bit for bit against forward_aud), which
must lie in 0.2 .. 0.8: a fixture whose ReLUs are all open or all shut would pin nothing.  No reference source is copied.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import make_golden as MG  # noqa: E402
from jegal_amd import synth  # noqa: E402

SEED = 20260
N = 29


def main():
    GestSync, _ = MG._import_reference()
    model = MG._load(GestSync(), synth.gestsync_state_dict(family="gauss"))
    x = torch.from_numpy(np.random.default_rng(SEED).standard_normal((N, 1, 80, 100)).astype(np.float32))
    with torch.no_grad():
        out = model.forward_aud(x)
        assert tuple(out.shape) == (N, 1024, 1), out.shape
        # replay for the active fractions
        names, active = [], []
        h = x
        net = model.net_aud
        for l in range(1, 7):
            conv = getattr(net, ("fc" if l == 6 else "conv") + str(l))
            h = torch.relu(getattr(net, "bn" + str(l))(conv(h)))
            names.append(("fc" if l == 6 else "conv") + str(l))
            active.append(float((h > 0).float().mean()))
            if hasattr(net, "mp" + str(l)):
                h = getattr(net, "mp" + str(l))(h)
        h = torch.relu(model.ff_aud.bn7(model.ff_aud.fc7(h)))
        names.append("fc7")
        active.append(float((h > 0).float().mean()))
        replay = model.ff_aud.fc8(h).squeeze(-1)
        assert torch.equal(replay, out), "the layer replay is not forward_aud"
        ref64 = model.double().forward_aud(x.double())
    rel = float((out.double() - ref64).norm() / ref64.norm())
    for n, a in zip(names, active):
        print(f"{n}: active {a:.3f}")
        assert 0.2 <= a <= 0.8, f"degenerate fixture: {n} has {a:.3f} of its units active"
    print(f"fp32 forward_aud vs its float64 evaluation: rel-L2 {rel:.2e}")
    path = os.path.join(MG.OUT, "gestsync_audio.npz")
    np.savez_compressed(path, seed=np.int64(SEED), out=out[:, :, 0].numpy().astype(np.float32), layers=np.asarray(names),
                        active=np.asarray(active, np.float32), ref_fp32_rel_l2=np.float64(rel))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
