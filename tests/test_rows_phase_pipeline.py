"""The regular row kernel's GEMM phases (k_step_rows, gemm_phase_x3) at the
smallest shapes at which their ring order, counted waits or bias offsets can
go wrong.  The bf16x3 phase reads its A fragments two k-steps ahead at W = 512
(one wave per SIMD) and retires each with a counted lgkmcnt wait; the other
widths read one ahead.  That changes no arithmetic, so the checks are the
parity checks of tests/test_gpu_parity.py.  (Two further changes were built
and measured slower; the cases that cover them — the mixed-depth
group and the 4-layer group for the bias staging — stay, since any later work
on the phase boundaries meets the same edges.)

Every case is a group of 8 fits trained for 3 epochs in both precisions and
compared fit by fit with oracle/siren_oracle.py (computed once per case and
shared by the two precisions).  Groups this small would take the K-split row
kernel in bf16x3 (at most 128 regular workgroups, rows_ks_for), so the tests
force the regular one with NERFHIP_ROWS_KS=0 and assert it from the group plan.

Tolerances are those of test_steps_match_reference, which the commit before
the change passes at these shapes (parameters within 2.5e-4 per step and
99.9 % of them within 1e-6, losses rtol 2e-5), and, for row_cos and the mean
cosine, of test_shapes_vs_oracle (atol 5e-3, 1e-3).

Worst deviations of the commit before the change at these cases, over the 8
fits (the changed kernel gives the same figures, its results being bitwise
equal): max |d param|, max relative loss error, max |d row_cos|

  case                       fp32                          bf16x3
  w256_l3_one_workgroup      4.2e-06  1.3e-07  2.1e-07     2.9e-06  1.3e-07  1.8e-07
  w256_l2_ragged             4.9e-06  1.3e-07  3.3e-07     5.6e-06  1.3e-07  3.0e-07
  w256_l1_l3_mixed           9.3e-06  1.2e-07  3.9e-07     1.1e-05  6.4e-08  3.9e-07
  w512_l2_two_passes         2.1e-05  1.2e-07  6.9e-07     1.4e-05  1.2e-07  4.8e-07
  w64_l1_n48                 3.2e-07  1.2e-07  1.2e-07     3.0e-07  1.2e-07  1.0e-07
  w128_l1_d64                1.6e-05  6.2e-08  3.1e-06     4.4e-06  6.2e-08  8.7e-07
  w256_l4_deepest            1.6e-05  6.3e-08  3.9e-07     1.8e-05  6.4e-08  5.1e-07

Every parameter was within 1e-6 in every case (fraction 1.0), and the mean
cosine within 6e-8.
"""

import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

import siren_oracle
from nerf_attention import SIREN, SIRENConfig, engine

ROOT = Path(__file__).resolve().parent.parent
EPOCHS = 3
FITS = 8
OMEGA = 30.0

# name -> (W, [L of each fit], N, D)
CASES = {
    "w256_l3_one_workgroup": (256, [3] * FITS, 64, 128),       # every phase, one workgroup
    "w256_l2_ragged": (256, [2] * FITS, 80, 128),              # ragged second workgroup
    "w256_l1_l3_mixed": (256, [1, 3] * (FITS // 2), 64, 128),  # per-fit bias offsets, L_max > L
    "w512_l2_two_passes": (512, [2] * FITS, 64, 128),          # two passes and the stash
    "w64_l1_n48": (64, [1] * FITS, 48, 128),                   # small KC, P > 1 DMA rounds
    "w128_l1_d64": (128, [1] * FITS, 64, 64),                  # d_head 64
    "w256_l4_deepest": (256, [4] * FITS, 64, 128),             # the deepest group the engine takes
}


@lru_cache(maxsize=None)
def _case(name):
    """(targets, configs, inits, oracle results) of a case; the oracle runs
    once and its results are never modified."""
    W, Ls, N, D = CASES[name]
    g = torch.Generator().manual_seed(1000 + W + N + D + sum(Ls))
    targets, cfgs, inits, refs = [], [], [], []
    for i, L in enumerate(Ls):
        t = torch.sin(torch.linspace(0, 7, N)[:, None] * torch.rand(1, D, generator=g) * 6) \
            + 0.1 * torch.randn(N, D, generator=g)
        cfg = SIRENConfig(W, L, OMEGA, f"{name}_{i}")
        torch.manual_seed(i)
        init = SIREN(cfg, D).flat_parameters()
        targets.append(t)
        cfgs.append(cfg)
        inits.append(init)
        refs.append(siren_oracle.fit(t, W, L, OMEGA, init, EPOCHS))
    return targets, cfgs, inits, refs


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", list(CASES))
def test_regular_rows_vs_oracle(gpu, monkeypatch, name, precision):
    targets, cfgs, inits, refs = _case(name)
    monkeypatch.setenv("NERFHIP_ROWS_KS", "0")
    specs = [engine.FitSpec(target=t, config=c, init=x) for t, c, x in zip(targets, cfgs, inits)]
    job = engine.FitJob(specs, EPOCHS, devices=[0], precision=precision)
    assert len(job.groups) == 1 and job.groups[0].n == FITS
    assert job.groups[0].plan()["rows_variant"] == "regular"
    job.launch()
    job.wait()
    worst = {"param": 0.0, "param_frac_1e-6": 1.0, "loss_rel": 0.0, "row_cos": 0.0, "cos": 0.0}
    outs = job.outputs()
    for out, ref in zip(outs, refs):
        dev = np.abs(out.params.cpu().numpy() - ref["params"].numpy())
        lr, lo = np.asarray(ref["losses"]), np.asarray(out.losses)
        worst["param"] = max(worst["param"], float(dev.max()))
        worst["param_frac_1e-6"] = min(worst["param_frac_1e-6"], float(np.mean(dev <= 1e-6)))
        worst["loss_rel"] = max(worst["loss_rel"], float(np.max(np.abs(lo - lr) / np.abs(lr))))
        worst["row_cos"] = max(worst["row_cos"],
                               float(np.max(np.abs(out.row_cos - ref["cosine_sims"]))))
        worst["cos"] = max(worst["cos"], abs(float(np.mean(out.row_cos)) - ref["final_cosine_mean"]))
    print(f"WORST {name} {precision} " + " ".join(f"{k}={v:.3e}" for k, v in worst.items()))
    for out, ref in zip(outs, refs):
        dev = np.abs(out.params.cpu().numpy() - ref["params"].numpy())
        assert dev.max() <= 2.5e-4 * EPOCHS, dev.max()          # <= 2·lr per step, ever
        assert np.mean(dev <= 1e-6) >= 0.999, np.mean(dev <= 1e-6)
        np.testing.assert_allclose(out.losses, ref["losses"], rtol=2e-5)
        np.testing.assert_allclose(out.row_cos, ref["cosine_sims"], atol=5e-3)
        assert abs(float(np.mean(out.row_cos)) - ref["final_cosine_mean"]) <= 1e-3


def test_w256_row_kernel_resources():
    """Two W = 256 bf16x3 row workgroups share a CU's 160 KiB of LDS, and the
    kernel's scratch stays within its documented 120 B per lane (host only:
    the built library's metadata).  Both are what keeps it at two waves per
    SIMD with nothing spilled inside the k-step loop."""
    sys.path.insert(0, str(ROOT / "tools"))
    import kernel_resources
    ks = kernel_resources.kernels()
    k = ks["void k_step_rows<256, 128, true, true>(nerfhip_detail::KArgs)"]
    assert 2 * k["group_segment_fixed_size"] <= 160 * 1024, k
    assert k["private_segment_fixed_size"] <= 120, k
