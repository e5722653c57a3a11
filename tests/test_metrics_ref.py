"""CPU tests of the evaluate feature: the fp64 oracle of metrics_ref.py against a scipy float64 restatement, the
CSV writers, the host refusals of ops.image_metrics that need no GPU, and the row formatting of the two evaluate
loops fed a stub metrics result."""
import csv
import re

import numpy as np
import pytest
import torch

import metrics_ref as mr

SHAPES = [(2, 2, 64, 48), (2, 1, 7, 9), (1, 2, 20, 16, 12)]


def _scipy_ssim(x, y):
    """skimage's structural_similarity (defaults, data_range 1) restated on float64 with uniform_filter."""
    from scipy.ndimage import uniform_filter
    npix = float(mr.WIN ** x.ndim)
    cov = npix / (npix - 1.0)
    f = lambda a: uniform_filter(a, size=mr.WIN)
    ux, uy = f(x), f(y)
    vx, vy, vxy = cov * (f(x * x) - ux * ux), cov * (f(y * y) - uy * uy), cov * (f(x * y) - ux * uy)
    s = ((2 * ux * uy + mr.C1) * (2 * vxy + mr.C2)) / ((ux ** 2 + uy ** 2 + mr.C1) * (vx + vy + mr.C2))
    pad = (mr.WIN - 1) // 2
    return float(s[tuple(slice(pad, n - pad) for n in s.shape)].mean())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", mr.MAKERS)
def test_oracle_agrees_with_uniform_filter_float64(kind, shape):
    gen, tgt = mr.make(kind, shape)
    assert gen.dtype == torch.float32 and tuple(gen.shape) == shape == tuple(tgt.shape)
    for clamp in (True, False):
        ref = mr.oracle(gen, tgt, clamp)
        g, t = (gen.clamp(0, 1), tgt.clamp(0, 1)) if clamp else (gen, tgt)
        g, t = g.double().numpy(), t.double().numpy()
        for i in range(shape[0]):
            want = np.mean([_scipy_ssim(g[i, c], t[i, c]) for c in range(shape[1])])
            assert abs(ref["ssim"][i] - want) <= 1e-10, (kind, shape, clamp, ref["ssim"][i], want)
            m = float(((g[i] - t[i]) ** 2).mean())
            assert abs(ref["mse"][i] - m) <= 1e-15 + 1e-13 * m
            assert abs(ref["psnr"][i] - 10 * np.log10(1 / max(m, 1e-12))) <= 1e-10
    if kind == "identical":
        assert np.all(ref["ssim"] == 1.0) and np.all(ref["mse"] == 0.0) and np.all(ref["psnr"] == 120.0)
    if kind == "out_of_range":
        assert not np.allclose(mr.oracle(gen, tgt, True)["mse"], mr.oracle(gen, tgt, False)["mse"])


def test_makers_have_the_property_they_are_named_for():
    shape = (1, 1, 40, 40)
    gen, tgt = mr.make("ct", shape)
    both_zero = (gen == 0) & (tgt == 0)
    assert both_zero.float().mean() > 0.2 and bool(((gen == 0) == (tgt == 0)).all())
    gen, tgt = mr.make("flat_bright", shape)
    assert float((gen - 0.97).abs().max()) < 1e-2
    gen, tgt = mr.make("out_of_range", shape)
    assert float(gen.min()) < 0 and float(gen.max()) > 1
    assert abs(float(mr.oracle(*mr.make("uniform", shape))["ssim"][0])) < 0.1
    a, b = mr.make("noisy", shape, seed=3), mr.make("noisy", shape, seed=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert np.isnan(mr.oracle(torch.rand(2, 1, 64), torch.rand(2, 1, 64))["ssim"]).all()


# ------------------------------------------------------------------ CSV writers
def _read(path):
    with open(path, newline="") as fh:
        return list(csv.reader(fh))


def test_summary_csv_appends_with_one_header_and_write_overwrites(tmp_path):
    from fmdiff.utils.sampling_utils import append_eval_metrics, write_eval_metrics
    root = tmp_path / "ckpt" / "run"     # created on demand
    row = {"samples": 4, "mse": "0.00100000", "psnr": "30.000000", "ssim": "", "ssim_enabled": True}
    p = append_eval_metrics(root, row)
    assert p == root / "eval_metrics.csv"
    append_eval_metrics(root, dict(row, samples=8))
    got = _read(p)
    assert got[0] == ["samples", "mse", "psnr", "ssim", "ssim_enabled"]
    assert [r[0] for r in got[1:]] == ["4", "8"] and got[1][4] == "True" and len(got) == 3
    assert write_eval_metrics(root, dict(row, samples=2)) == p
    got = _read(p)
    assert len(got) == 2 and got[1][0] == "2"


def test_per_image_csv_union_of_keys_and_empty_rows(tmp_path):
    from fmdiff.utils.sampling_utils import append_per_image_eval_metrics
    p = append_per_image_eval_metrics(tmp_path, [])
    assert p == tmp_path / "eval_metrics_per_image.csv" and p.read_text() == ""
    rows = [{"sample_index": 0, "mse": "1"}, {"sample_index": 1, "psnr": "2", "mse": "3"}, {"extra": "x"}]
    append_per_image_eval_metrics(tmp_path, rows)
    got = _read(p)
    assert got[0] == ["sample_index", "mse", "psnr", "extra"]
    assert got[1:] == [["0", "1", "", ""], ["1", "3", "2", ""], ["", "", "", "x"]]
    append_per_image_eval_metrics(tmp_path, rows[:1])            # overwrites
    assert _read(p) == [["sample_index", "mse"], ["0", "1"]]
    append_per_image_eval_metrics(tmp_path, [])                  # an existing file is left alone
    assert _read(p) == [["sample_index", "mse"], ["0", "1"]]


# ------------------------------------------------------------------ host refusals
def test_image_metrics_host_refusals():
    from fmdiff.runtime import ops
    z = torch.zeros
    with pytest.raises(NotImplementedError):
        ops.image_metrics(z(1, 1, 7, 7, 7, 7), z(1, 1, 7, 7, 7, 7))
    with pytest.raises(ValueError, match=r"^win_size exceeds image extent"):
        ops.image_metrics(z(1, 1, 6, 9), z(1, 1, 6, 9))
    with pytest.raises(ValueError, match=r"^win_size exceeds image extent"):
        ops.image_metrics(z(1, 1, 9, 9, 5), z(1, 1, 9, 9, 5))
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.image_metrics(z(1, 1, 8, 8), z(1, 1, 8, 9))
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        ops.image_metrics(z(1, 1, 8, 8), z(1, 1, 8, 8))
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        ops.image_metrics(z(2, 1, 64), z(2, 1, 64))


def test_compute_ssim_sample_reference_conditions():
    from fmdiff.utils.evaluation_utils import compute_ssim_sample
    calls = []

    def fn(a, b, channel_axis, data_range):
        assert channel_axis is None and data_range == 1.0 and a.dtype == np.float32
        calls.append(a.shape)
        return 0.25 * len(calls)

    assert compute_ssim_sample(torch.zeros(2, 8, 8), torch.zeros(2, 8, 9), fn) is None
    assert compute_ssim_sample(torch.zeros(8), torch.zeros(8), fn) is None
    assert compute_ssim_sample(torch.zeros(2, 8, 8), torch.zeros(2, 8, 8), fn) == pytest.approx(0.375)
    assert calls == [(8, 8), (8, 8)]
    assert compute_ssim_sample(torch.zeros(8, 8), torch.zeros(8, 8), fn) == 0.75 and calls[-1] == (8, 8)
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        compute_ssim_sample(torch.zeros(2, 8, 8), torch.zeros(2, 8, 8))


# ------------------------------------------------------------------ evaluate loops on a stub metrics result
PER_IMAGE = {"mse": r"^\d+\.\d{8}$", "psnr": r"^-?\d+\.\d{6}$", "ssim": r"^-?\d+\.\d{6}$"}
SUMMARY_KEYS = ["samples", "mse", "psnr", "ssim", "ssim_enabled", "model_seconds", "model_samples_per_second",
                "model_seconds_per_sample", "model_calls"]
PER_IMAGE_KEYS = ["sample_index", "img_id", "img_path", "mse", "psnr", "ssim"]


def _stub_metrics(monkeypatch, seen):
    from fmdiff.runtime import ops

    def image_metrics(gen, tgt, clamp=True):
        seen.append((tuple(gen.shape), clamp))
        ref = mr.oracle(gen, tgt, clamp)
        st = torch.tensor(np.stack([ref["mse"], ref["psnr"], ref["ssim"]]))
        return ops.ImageMetrics(st[0], st[1], st[2], st)

    monkeypatch.setattr(ops, "image_metrics", image_metrics)


def _batches(shape, with_image=True):
    g = torch.Generator().manual_seed(5)
    out = []
    for b in range(2):
        samples = []
        for j in range(2):
            s = {"target": torch.rand(shape, generator=g), "img_id": f"id{2 * b + j}", "img_path": f"/d/{2 * b + j}.png"}
            if with_image:
                s["image"] = torch.rand(shape, generator=g)
            samples.append(s)
        out.append(([10 + 2 * b, 11 + 2 * b], samples))
    return out


def _check_rows(row, rows, seen_pairs, clamp):
    assert list(row) == SUMMARY_KEYS and all(list(r) == PER_IMAGE_KEYS for r in rows)
    assert [r["sample_index"] for r in rows] == [10, 11, 12, 13] and rows[2]["img_id"] == "id2"
    assert rows[3]["img_path"] == "/d/3.png"
    want = [mr.oracle(g, t, clamp) for g, t in seen_pairs]
    flat = {k: np.concatenate([w[k] for w in want]) for k in ("mse", "psnr", "ssim")}
    for i, r in enumerate(rows):
        for k, pat in PER_IMAGE.items():
            assert re.match(pat, r[k]), (k, r[k])
            assert abs(float(r[k]) - flat[k][i]) <= 1e-6
    assert row["samples"] == 4 and row["ssim_enabled"] is True
    for k in ("mse", "psnr", "ssim"):
        assert abs(float(row[k]) - flat[k].mean()) <= 1e-6


def test_evaluate_diffusion_rows_from_a_stub(monkeypatch, tmp_path):
    from fmdiff.pipelines.samplers import evaluate_diffusion
    from fmdiff.utils.model_utils import diffusion_utils as DU
    seen, calls, pairs = [], [], []
    _stub_metrics(monkeypatch, seen)

    def decode(model, tr, mc, device, shape, cond, **kw):
        calls.append((tuple(shape), None if cond is None else tuple(cond.shape), kw))
        kw["timing"]["model_seconds"] += 0.5
        kw["timing"]["model_calls"] += 3
        return kw["reference_batch"] + (0.05 * cond if cond is not None else 0.03) - 0.02

    monkeypatch.setattr(DU, "decode_diffusion_batch", decode)
    cfg = {"training": {"conditioning": "Concatenate"}, "model": {}}
    row, rows = evaluate_diffusion(object(), cfg, _batches((1, 9, 10)), "cpu", num_inference_steps=3, last_n_steps=2,
                                   scheduler="ddim", metrics_root=tmp_path,
                                   on_batch=lambda i, g, t: pairs.append((g, t)))
    assert seen == [((2, 1, 9, 10), True)] * 2
    shape, cshape, kw = calls[0]
    assert shape == cshape == (2, 1, 9, 10) and kw["init_from_reference"] is True and kw["last_n_steps"] == 2
    assert kw["num_inference_steps"] == 3 and kw["start_step"] is None and kw["scheduler_override"] == "ddim"
    _check_rows(row, rows, pairs, True)
    assert row["model_calls"] == 6 and row["model_seconds"] == "1.000000"
    assert row["model_samples_per_second"] == "4.000000" and row["model_seconds_per_sample"] == "0.25000000"
    got = _read(tmp_path / "eval_metrics.csv")
    assert got[0] == SUMMARY_KEYS and got[1][4] == "True" and len(got) == 2
    got = _read(tmp_path / "eval_metrics_per_image.csv")
    assert got[0] == PER_IMAGE_KEYS and len(got) == 5
    # no conditioning when a sample lacks its image, or when the mode takes none
    calls.clear()
    b = _batches((1, 9, 10))
    del b[0][1][1]["image"]
    evaluate_diffusion(object(), {"training": {}, "model": {"conditioning": "attention"}}, b, "cpu")
    evaluate_diffusion(object(), {"training": {}, "model": {}}, b[1:], "cpu", start_step=400)
    assert [c[1] for c in calls] == [None, (2, 1, 9, 10), None]
    assert [c[2]["init_from_reference"] for c in calls] == [False, False, True] and calls[2][2]["start_step"] == 400
    with pytest.raises(RuntimeError, match=r"^No samples available for evaluation\.$"):
        evaluate_diffusion(object(), cfg, [], "cpu")


def test_evaluate_autoencoder_rows_and_signals_from_a_stub(monkeypatch, tmp_path):
    from fmdiff.pipelines.samplers import evaluate_autoencoder
    seen, pairs = [], []
    _stub_metrics(monkeypatch, seen)

    class Model:
        def image_to_model_range(self, x):
            return 2 * x - 1

        def forward(self, x, sample_posterior=True):
            assert sample_posterior is False
            return 0.9 * x, None

        __call__ = forward

        def raw_output_to_image(self, x, recon_type="l1"):
            assert recon_type == "mse"
            return (x + 1) / 2

    cfg = {"training": {"recon_type": "mse"}}
    row, rows = evaluate_autoencoder(Model(), cfg, _batches((1, 9, 10), False), "cpu", metrics_root=tmp_path,
                                     on_batch=lambda i, g, t: pairs.append((g, t)))
    assert seen == [((2, 1, 9, 10), False)] * 2
    _check_rows(row, rows, pairs, False)
    assert row["model_calls"] == 2
    assert _read(tmp_path / "eval_metrics.csv")[0] == SUMMARY_KEYS
    # [N, C, L] signals: empty SSIM cells and an empty SSIM summary
    row, rows = evaluate_autoencoder(Model(), cfg, _batches((1, 64), False), "cpu")
    assert all(r["ssim"] == "" and re.match(PER_IMAGE["mse"], r["mse"]) for r in rows) and row["ssim"] == ""
    with pytest.raises(RuntimeError, match=r"^No samples available for evaluation\.$"):
        evaluate_autoencoder(Model(), cfg, [], "cpu")
