"""GPU tests of the image-metrics kernel (csrc/metrics.hip) through ops.image_metrics, compute_ssim_sample and the
two evaluate loops.

Kernel level: every input maker of metrics_ref.py on every shape of SHAPES_2D / SHAPES_3D and both clamp settings
against the fp64 oracle: |ssim - ssim64| <= 1e-9, mse within 1e-12 relative, psnr within 1e-9 (DESIGN.md
section 4, "Image metrics: fp64 bound").  The 2-D tile holds 32 x 32 window positions, so a 37 x 37 image is one
position short of a full tile and a 39 x 39 image one past it; 45 x 70 has three tiles along x.  The 3-D tile
holds 8 x 8 x 16 positions: 20 x 16 x 12 (D x H x W) has 14 x 10 x 6 positions, two tiles along y.  Outputs and
workspace sit in sentinel buffers whose guards must come back untouched.
"""
import csv
import re

import numpy as np
import pytest
import torch

import metrics_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
TILE = 32   # window positions per 2-D tile edge (csrc/metrics.hip Tile<2>)

SHAPES_2D = [(1, 1, 7, 7), (2, 1, 7, 9), (3, 2, 45, 70), (2, 1, TILE + 6 - 1, TILE + 6 - 1),
             (2, 1, TILE + 6 + 1, TILE + 6 + 1)]
SHAPES_3D = [(1, 1, 7, 7, 7), (2, 1, 9, 8, 7), (1, 2, 20, 16, 12)]
_refs = {}


def _case(kind, shape):
    """Device inputs and the fp64 oracle for both clamp settings, computed once and shared (never modified)."""
    if (kind, shape) not in _refs:
        gen, tgt = mr.make(kind, shape)
        _refs[kind, shape] = (gen.to(DEV), tgt.to(DEV), {c: mr.oracle(gen, tgt, c) for c in (True, False)})
    return _refs[kind, shape]


def _run(gen, tgt, clamp):
    """ops.image_metrics with the [3, N] output and the workspace inside NaN-filled guarded buffers."""
    from fmdiff import _lib
    from fmdiff.runtime import ops
    N, sp = gen.shape[0], tuple(gen.shape[2:])
    need = int(_lib.lib().fmd_image_metrics_workspace(N, gen.shape[1], *((0,) * (3 - len(sp)) + sp)))
    assert need > 0 and need % 16 == 0
    obuf = torch.full((3 * N + 2 * GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    wbuf = torch.full((need + 2 * GUARD * 8,), 0xA5, dtype=torch.uint8, device=DEV)
    out = obuf[GUARD:GUARD + 3 * N].view(3, N)
    m = ops.image_metrics(gen, tgt, clamp, out=out, ws=wbuf[GUARD * 8:GUARD * 8 + need])
    torch.cuda.synchronize()
    assert bool(torch.isnan(torch.cat([obuf[:GUARD], obuf[-GUARD:]])).all()), "output guard overwritten"
    assert bool((torch.cat([wbuf[:GUARD * 8], wbuf[-GUARD * 8:]]) == 0xA5).all()), "workspace guard overwritten"
    assert m.mse.data_ptr() == out.data_ptr() and m.stacked.dtype == torch.float64 and m.ssim.shape == (N,)
    return m


def _host(m):
    return tuple(v.cpu().numpy() for v in (m.mse, m.psnr, m.ssim))


@pytest.mark.parametrize("shape", SHAPES_2D + SHAPES_3D, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", mr.MAKERS)
def test_image_metrics_against_fp64(kind, shape):
    gen, tgt, refs = _case(kind, shape)
    for clamp in (True, False):
        got = _host(_run(gen, tgt, clamp))
        worst = mr.check(got, refs[clamp], f"{kind} {shape} clamp={clamp}")
        print(f"{kind} {shape} clamp={clamp}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
              + f"; ssim {got[2].tolist()}")
        if kind == "identical":
            assert np.all(got[2] == 1.0) and np.all(got[0] == 0.0) and np.all(got[1] == 120.0), got


@pytest.mark.parametrize("shape", [(3, 2, 45, 70), (3, 1, 20, 16, 12)], ids=["2d", "3d"])
def test_deterministic_and_independent_of_the_batch(shape):
    gen, tgt = (v.to(DEV) for v in mr.make("noisy", shape, seed=1))
    a, b = _run(gen, tgt, True).stacked.clone(), _run(gen, tgt, True).stacked.clone()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    for i in range(shape[0]):
        one = _run(gen[i:i + 1].contiguous(), tgt[i:i + 1].contiguous(), True).stacked
        assert torch.equal(one[:, 0].view(torch.int64), a[:, i].view(torch.int64)), i


@pytest.mark.parametrize("shape", [(3, 2, 45, 70), (3, 1, 20, 16, 12)], ids=["2d", "3d"])
@pytest.mark.parametrize("clamp", [True, False])
def test_nan_reaches_its_own_image_only(shape, clamp):
    gen, tgt = (v.to(DEV) for v in mr.make("out_of_range", shape, seed=2))
    clean = _run(gen, tgt, clamp).stacked.clone()
    bad = gen.clone()
    bad[(1, shape[1] - 1) + tuple(s // 2 for s in shape[2:])] = float("nan")
    got = _run(bad, tgt, clamp).stacked
    assert bool(torch.isnan(got[:, 1]).all()), got[:, 1].tolist()
    for i in (0, 2):
        assert torch.equal(got[:, i].view(torch.int64), clean[:, i].view(torch.int64)), i


def test_signals_get_mse_and_psnr_and_nan_ssim():
    for shape in [(2, 1, 64), (2, 3, 5000)]:     # the second spans several partial blocks per image
        gen, tgt = mr.make("out_of_range", shape)
        for clamp in (True, False):
            got = _host(_run(gen.to(DEV), tgt.to(DEV), clamp))
            assert np.isnan(got[2]).all()
            mr.check(got, mr.oracle(gen, tgt, clamp), f"signal {shape} clamp={clamp}")


def test_refusals():
    from fmdiff import _lib
    from fmdiff.runtime import ops
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(NotImplementedError):
        ops.image_metrics(z(1, 1, 7, 7, 7, 7), z(1, 1, 7, 7, 7, 7))
    for s in [(1, 1, 6, 9), (1, 1, 9, 6), (1, 1, 6, 9, 9), (1, 1, 9, 9, 5)]:
        with pytest.raises(ValueError, match=r"^win_size exceeds image extent"):
            ops.image_metrics(z(*s), z(*s))
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.image_metrics(z(1, 1, 8, 8), z(1, 1, 8, 9))
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        ops.image_metrics(torch.zeros(1, 1, 8, 8), z(1, 1, 8, 8))
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        ops.image_metrics(z(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))
    with pytest.raises(RuntimeError, match="contiguous fp32"):
        ops.image_metrics(z(1, 1, 8, 8).double(), z(1, 1, 8, 8).double())
    L = _lib.lib()
    for args in [(0, 1, 0, 8, 8), (1, 0, 0, 8, 8), (1, 1, 0, 6, 8), (1, 1, 0, 8, 6), (1, 1, 6, 8, 8), (1, 1, 8, 8, 6),
                 (1, 1, 8, 0, 8)]:
        assert L.fmd_image_metrics_workspace(*args) == -1, args
    a, o = z(1, 1, 8, 8), torch.zeros(3, device=DEV, dtype=torch.float64)
    w = torch.zeros(64, device=DEV, dtype=torch.uint8)
    assert L.fmd_image_metrics(a.data_ptr(), a.data_ptr(), 1, 1, 0, 6, 8, 1, w.data_ptr(), o.data_ptr(), o.data_ptr(),
                               o.data_ptr(), None) == -1
    assert L.fmd_image_metrics_workspace(1, 1, 0, 8, 8) == 16


def test_compute_ssim_sample_uses_the_kernel():
    from fmdiff.utils.evaluation_utils import compute_ssim_sample
    gen, tgt = mr.make("noisy", (1, 2, 16, 16))
    want = mr.oracle(gen, tgt, False)["ssim"][0]
    got = compute_ssim_sample(gen[0].to(DEV), tgt[0].to(DEV))
    assert isinstance(got, float) and abs(got - want) <= mr.SSIM_TOL
    one = compute_ssim_sample(gen[0, 0].to(DEV), tgt[0, 0].to(DEV))        # [H, W]: one image
    assert abs(one - mr.oracle(gen[:, :1], tgt[:, :1], False)["ssim"][0]) <= mr.SSIM_TOL
    assert compute_ssim_sample(gen[0].to(DEV), tgt[0, :, :15].to(DEV)) is None


# ------------------------------------------------------------------ end to end
FORMATS = {"mse": r"^\d+\.\d{8}$", "psnr": r"^-?\d+\.\d{6}$", "ssim": r"^-?\d+\.\d{6}$"}
SUMMARY_KEYS = ["samples", "mse", "psnr", "ssim", "ssim_enabled", "model_seconds", "model_samples_per_second",
                "model_seconds_per_sample", "model_calls"]
PER_IMAGE_KEYS = ["sample_index", "img_id", "img_path", "mse", "psnr", "ssim"]


def _batches(size, with_image):
    g = torch.Generator().manual_seed(11)
    out = []
    for b in range(2):
        samples = []
        for j in range(2):
            s = {"target": torch.rand(1, size, size, generator=g), "img_id": f"case{2 * b + j}",
                 "img_path": f"data/{2 * b + j}.npy"}
            if with_image:
                s["image"] = torch.rand(1, size, size, generator=g)
            samples.append(s)
        out.append(([2 * b, 2 * b + 1], samples))
    return out


def _read(path):
    with open(path, newline="") as fh:
        return list(csv.DictReader(fh))


def _check_end_to_end(row, rows, captured, clamp, root):
    assert len(captured) == 2 and all(g.device.type == "cuda" and g.shape == t.shape for g, t in captured)
    flat = {k: np.concatenate([mr.oracle(g, t, clamp)[k] for g, t in captured]) for k in FORMATS}
    assert list(row) == SUMMARY_KEYS and len(rows) == 4 and all(list(r) == PER_IMAGE_KEYS for r in rows)
    for i, r in enumerate(rows):
        assert r["sample_index"] == i and r["img_id"] == f"case{i}" and r["img_path"] == f"data/{i}.npy"
        for k, pat in FORMATS.items():
            assert re.match(pat, r[k]), (k, r[k])
            assert abs(float(r[k]) - flat[k][i]) <= 1e-6, (k, r[k], flat[k][i])
    assert row["samples"] == 4 and row["ssim_enabled"] is True and row["model_calls"] > 0
    for k in FORMATS:
        assert re.match(FORMATS[k], row[k]) and abs(float(row[k]) - flat[k].mean()) <= 1e-6, (k, row[k])
    assert float(row["model_seconds"]) > 0 and float(row["model_samples_per_second"]) > 0
    summary = _read(root / "eval_metrics.csv")
    assert len(summary) == 1 and list(summary[0]) == SUMMARY_KEYS
    assert summary[0]["ssim_enabled"] == "True" and summary[0]["samples"] == "4" and summary[0]["mse"] == row["mse"]
    per_image = _read(root / "eval_metrics_per_image.csv")
    assert len(per_image) == 4 and list(per_image[0]) == PER_IMAGE_KEYS
    assert [r["mse"] for r in per_image] == [r["mse"] for r in rows]
    print(f"summary {row}")


def test_evaluate_diffusion_end_to_end(tmp_path):
    from fmdiff.models.generators import DiffusionUNetFactory
    from fmdiff.pipelines.samplers import evaluate_diffusion
    from oracle import spec as S
    from oracle import unet as U
    ucfg = {"block_out_channels": [32, 64], "layers_per_block": 1, "attention_resolutions": []}
    model = DiffusionUNetFactory().build(ucfg, "concatenate", 1).to(DEV).eval()
    model.load_state_dict(U.seeded_state_dict(S.derive_spec(ucfg, "concatenate", 1), 7))
    cfg = {"training": {"conditioning": "concatenate", "channels": 1, "num_train_timesteps": 1000},
           "model": {"unet": ucfg, "scheduler": {"name": "flow_match_euler"}}}
    captured = []
    row, rows = evaluate_diffusion(model, cfg, _batches(16, True), torch.device(DEV), num_inference_steps=2,
                                   metrics_root=tmp_path, on_batch=lambda i, g, t: captured.append((g, t)))
    assert all(g.shape == (2, 1, 16, 16) for g, _ in captured)
    _check_end_to_end(row, rows, captured, True, tmp_path)
    assert row["model_calls"] == 4       # 2 steps x 2 batches


def test_evaluate_autoencoder_end_to_end(tmp_path):
    import json
    import os
    import warnings

    from fmdiff.models.vae import AutoencoderKL
    from fmdiff.pipelines.samplers import evaluate_autoencoder
    G = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vae_golden.pt"),
                   weights_only=True)
    vcfg = json.loads(bytes(G["cfg_json"].tolist()).decode())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vae = AutoencoderKL(**vcfg)
    vae.load_state_dict(G["state"])
    vae = vae.to(DEV).eval()
    captured = []
    row, rows = evaluate_autoencoder(vae, {"training": {"recon_type": "l1"}}, _batches(32, False), torch.device(DEV),
                                     metrics_root=tmp_path, on_batch=lambda i, g, t: captured.append((g, t)))
    assert all(g.shape == (2, 1, 32, 32) for g, _ in captured)
    _check_end_to_end(row, rows, captured, False, tmp_path)
    assert row["model_calls"] == 2
