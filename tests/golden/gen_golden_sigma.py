"""Generate tests/golden/sigma/golden_spring_s12_sigma2.npz: gen_golden.py's
spring_s12 run of the REFERENCE with ``log_sig = 2.0`` set on the reference
model (its decoder comment, nn/network/physics_models.py:155-161, invites
that).  Same machinery, same contents as golden_spring_s12.npz; nothing of the
reference is stored but what it computed.

The fixture lives in its own folder: helpers.GOLDEN globs golden/golden_*.npz
into the sigma = 1 tests, which must not pick it up.

Run where the reference is available:   python tests/golden/gen_golden_sigma.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as G  # noqa: E402

LOG_SIG = 2.0
NAME = "spring_s12"


def main():
    G._install_shims()
    sys.path.insert(0, G.REF)
    torch.set_num_threads(4)
    from nn.network.physics_models import PhysicsNet

    init = PhysicsNet.__init__

    def init_sigma(self, *a, **k):
        init(self, *a, **k)
        self.log_sig = LOG_SIG

    PhysicsNet.__init__ = init_sigma
    try:
        o = G.run_config(NAME)
    finally:
        PhysicsNet.__init__ = init
    o["log_sig"] = np.float64(LOG_SIG)
    os.makedirs(os.path.join(HERE, "sigma"), exist_ok=True)
    path = os.path.join(HERE, "sigma", f"golden_{NAME}_sigma2.npz")
    np.savez_compressed(path, **o)
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.0f} kB) train={o['loss_train']:.4f} "
          f"recons={o['loss_recons']:.4f} extrap={o['loss_extrap']:.4f}")


if __name__ == "__main__":
    main()
