"""CPU checks of the VAE trainer loop's host side (``fmdiff.pipelines.train.vae_lib.train``): the micro-batch
policy, the metrics header, the batch order, the picture and checkpoint helpers and what is refused by name."""
import json
import os
import time

import numpy as np
import pytest
import torch

MODEL = dict(model_type="vae", latent_type="kl", in_channels=1, out_channels=1, resolution=16, base_ch=32,
             down_channels=[32, 32], num_res_blocks=1, attn_resolutions=[], z_channels=4, embed_dim=4,
             use_attention=False, attn_heads=4, attn_dim_head=8)


class Items(torch.utils.data.Dataset):
    def __init__(self, n, seed=0):
        self.x = torch.rand(n, 1, 16, 16, generator=torch.Generator().manual_seed(seed))

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return {"target": self.x[i], "index": i}


def _config(tmp_path, **training):
    path = tmp_path / "cfg.json"
    tr = dict(output_dir=str(tmp_path / "run"), batch_size=4, num_workers=0, epochs=1, seed=3, **training)
    path.write_text(json.dumps({"model": MODEL, "training": tr}))
    return path


def test_train_without_a_dataset_points_at_the_design_notes():
    from fmdiff.pipelines.train import vae_lib
    with pytest.raises(NotImplementedError, match="DESIGN") as e:
        vae_lib.train(None, "this file is never read.json")
    assert '{"target": tensor}' in str(e.value)


def test_micro_batch_policy():
    from fmdiff.pipelines.train.vae_lib import OOM_DISABLED_MESSAGE, is_out_of_memory, next_micro_batch
    err = RuntimeError("HIP out of memory. Tried to allocate 2.00 GiB")
    assert is_out_of_memory(err) and is_out_of_memory(RuntimeError("CUDA OUT OF MEMORY"))
    assert not is_out_of_memory(RuntimeError("an illegal memory access")) and not is_out_of_memory(ValueError(str(err)))
    cur, seen = 8, []
    while cur > 1:
        cur = next_micro_batch(cur, True, err)
        seen.append(cur)
    assert seen == [4, 2, 1]
    with pytest.raises(RuntimeError) as e:
        next_micro_batch(1, True, err)
    assert e.value is err                                    # nothing left to halve: the error itself
    assert next_micro_batch(7, True) == 3 and next_micro_batch(3, True) == 1
    with pytest.raises(RuntimeError) as e:
        next_micro_batch(8, False, err)
    assert str(e.value) == OOM_DISABLED_MESSAGE and e.value.__cause__ is err
    assert OOM_DISABLED_MESSAGE == ("The current batch size is too large, please set it to a lower value or enable "
                                    "microbatching.")


def test_micro_batch_warning_counts_the_chunks():
    from fmdiff.pipelines.train.vae_lib import micro_batch_warning
    assert micro_batch_warning(2, 4) == ("The maximum batch size for the current configuration is 2; training with 2 "
                                         "micro batches of size 2 for gradient accumulation.")
    assert "3 micro batches of size 3" in micro_batch_warning(3, 8)


@pytest.mark.parametrize("tr,want", [
    ({}, ["loss", "recon", "kl", "vq"]),                                         # the defaults: reg kl, codebook 1
    ({"reg_type": "kl", "codebook_weight": 0.0}, ["loss", "recon", "kl"]),
    ({"reg_type": "vq", "codebook_weight": 0.0}, ["loss", "recon", "vq"]),
    ({"reg_type": "vq", "kl_weight": 1e-3, "codebook_weight": 0.0}, ["loss", "recon", "kl", "vq"]),
    ({"reg_type": "none", "codebook_weight": 0.0}, ["loss", "recon"]),
    ({"reg_type": "kl", "codebook_weight": 0.0, "perceptual_weight": 0.1}, ["loss", "recon", "kl", "perceptual"]),
    ({"reg_type": "vq", "gan_weight": 0.5}, ["loss", "recon", "vq", "g_gan", "d_gan"]),
    ({"perceptual_weight": 1.0, "gan_weight": 0.1}, ["loss", "recon", "kl", "vq", "perceptual", "g_gan", "d_gan"]),
])
def test_metrics_keys_and_header(tr, want):
    from fmdiff.pipelines.train.vae_lib import metrics_header, metrics_keys
    assert metrics_keys(tr) == want
    assert metrics_header(tr) == "epoch," + ",".join(want) + "\n"


def _grid_formula(t, rows, cols):
    """The issue's formula, written with loops: clamp, 1 -> 3 channels, times 255, clip, truncate, HWC."""
    t = t[: rows * cols].clamp(0.0, 1.0)
    n, c, h, w = t.shape
    out = np.zeros((rows * h, cols * w, 3 if c == 1 else c), dtype=np.uint8)
    for r in range(rows):
        for q in range(cols):
            img = t[r * cols + q]
            if c == 1:
                img = img.expand(3, h, w)
            out[r * h:(r + 1) * h, q * w:(q + 1) * w] = (img.numpy() * 255.0).clip(0, 255).astype(np.uint8).transpose(1, 2, 0)
    return out


def test_make_grid_is_the_formula():
    from fmdiff.utils import make_grid
    g = torch.Generator().manual_seed(1)
    rgb = torch.rand(7, 3, 5, 6, generator=g)
    wild = torch.randn(6, 3, 4, 4, generator=g) * 2.0          # below 0 and above 1
    wild[0, 0, 0, 0], wild[0, 0, 0, 1] = 1.0, 0.0
    gray = torch.rand(20, 1, 3, 2, generator=g)
    for t, rows, cols in ((rgb, 2, 3), (wild, 3, 2), (gray, 4, 5), (gray, 1, 1)):
        got = make_grid(t, rows, cols)
        assert got.dtype == np.uint8 and got.shape == (rows * t.shape[2], cols * t.shape[3], 3)
        assert np.array_equal(got, _grid_formula(t, rows, cols))
    assert make_grid(wild, 3, 2)[0, 0, 0] == 255 and make_grid(wild, 3, 2)[0, 1, 0] == 0
    assert (make_grid(gray, 4, 5)[..., 0] == make_grid(gray, 4, 5)[..., 2]).all()
    with pytest.raises(ValueError, match="Need at least 20 images to build the grid, found 7"):
        make_grid(rgb, 4, 5)


def test_save_image_and_loop_grid_bytes(tmp_path):
    """``save_image`` writes what ``make_grid`` made, and the FM loop's ``_save_grid`` still writes the pixels of
    its former private formula."""
    from PIL import Image
    from fmdiff.pipelines.train.loop import _save_grid
    from fmdiff.utils import make_grid, save_image
    t = torch.rand(5, 1, 4, 6, generator=torch.Generator().manual_seed(2)) * 1.2 - 0.1
    save_image(make_grid(t, 2, 2), tmp_path / "a" / "g.png")
    assert np.array_equal(np.asarray(Image.open(tmp_path / "a" / "g.png")), _grid_formula(t, 2, 2))
    _save_grid(t, tmp_path / "b.png")                          # 5 images: 2 x 2
    assert np.array_equal(np.asarray(Image.open(tmp_path / "b.png")), _grid_formula(t, 2, 2))


def test_latent_shape():
    from fmdiff.utils import latent_shape
    base = dict(embed_dim=4, resolution=64)
    assert latent_shape(dict(base, down_channels=[32, 64, 64])) == (4, 16, 16)
    assert latent_shape(dict(base, ch_mult=[1, 2, 4, 4])) == (4, 8, 8)
    assert latent_shape(dict(base, ch_mult=[1, 2], down_channels=[8, 8, 8, 8], spatial_dims=2)) == (4, 8, 8)
    assert latent_shape(dict(base, spatial_dims=1, down_channels=[32, 32])) == (4, 32)
    assert latent_shape(dict(base, spatial_dims=3, ch_mult=(1, 2, 4))) == (4, 16, 16, 16)
    assert latent_shape(dict(embed_dim=3, resolution=16, down_channels=[32])) == (3, 16, 16)
    with pytest.raises(KeyError):
        latent_shape(base)


def test_latest_checkpoint(tmp_path):
    from fmdiff.utils import latest_checkpoint
    assert latest_checkpoint(tmp_path) is None
    (tmp_path / "other.pt").write_bytes(b"x")
    assert latest_checkpoint(tmp_path) == tmp_path / "other.pt"
    now = time.time()
    for name, age in (("vae_best.pt", 50), ("vae_last.pt", 100), ("newer_but_unnamed.pt", 0)):
        (tmp_path / name).write_bytes(b"x")
        os.utime(tmp_path / name, (now - age, now - age))
    assert latest_checkpoint(tmp_path) == tmp_path / "vae_best.pt"     # the newer of the two named ones
    os.utime(tmp_path / "vae_last.pt", (now - 10, now - 10))
    assert latest_checkpoint(str(tmp_path)) == tmp_path / "vae_last.pt"


def test_prepare_eval_batch():
    from fmdiff.utils import prepare_eval_batch
    ds = Items(9)
    a = prepare_eval_batch(ds, 5, torch.device("cpu"), seed=4)
    b = prepare_eval_batch(ds, 5, torch.device("cpu"), seed=4)
    assert a.shape == (5, 1, 16, 16) and torch.equal(a, b)
    assert prepare_eval_batch(ds, 20, torch.device("cpu"), seed=4).shape[0] == 9
    with pytest.raises(RuntimeError, match="empty"):
        prepare_eval_batch(Items(0), 5, torch.device("cpu"))


def test_epoch_order_depends_on_seed_and_epoch_only():
    from fmdiff.pipelines.train.vae_lib import _EpochLoader, epoch_order
    ds = Items(11)

    def visited(loader, epoch):
        loader.set_epoch(epoch)
        return [int(i) for b in loader for i in b["index"]]

    a = _EpochLoader(ds, 4, 0, 5, pin_memory=False)
    first = {e: visited(a, e) for e in (1, 2, 3)}
    for e, order in first.items():
        assert sorted(order) == list(range(11)) and order == epoch_order(11, 5, e)
    assert first[1] != first[2] != first[3]
    # another loader, after other draws from the global stream, started at epoch 3 as a resumed run would
    torch.manual_seed(99)
    torch.rand(1000)
    b = _EpochLoader(ds, 4, 0, 5, pin_memory=False)
    assert visited(b, 3) == first[3] and visited(b, 2) == first[2]
    state = torch.random.get_rng_state()
    visited(b, 1)
    assert torch.equal(torch.random.get_rng_state(), state)          # and it leaves the global stream alone
    assert visited(_EpochLoader(ds, 4, 0, 6, pin_memory=False), 1) != first[1]
    assert visited(_EpochLoader(ds, 4, 0, None, pin_memory=False), 1) == epoch_order(11, 0, 1)
    sizes = [len(b["index"]) for b in a]
    assert sizes == [4, 4, 3]


@pytest.mark.parametrize("key,value", [("use_amp", True), ("disc_device", "cuda:1"), ("perceptual_device", "cuda:1")])
def test_unbuilt_settings_are_refused_by_name(tmp_path, key, value):
    from fmdiff.pipelines.train import vae_lib
    path = _config(tmp_path, **{key: value})
    with pytest.raises(NotImplementedError, match=key):
        vae_lib.train(Items(4), path)
    assert not (tmp_path / "run_run1").exists()                       # refused before anything is written


def test_a_cpu_device_is_refused(tmp_path):
    from fmdiff.pipelines.train import vae_lib
    path = _config(tmp_path, manual_device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        vae_lib.train(Items(4), path)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vae_lib.debug_visual_only(Items(4), path, tmp_path / "none.pt")


def test_perceptual_weights_are_never_downloaded(tmp_path):
    """Without ``perceptual=`` and without ``training.perceptual_weights`` the answer names both ways."""
    from fmdiff.pipelines.train.vae_lib import _build_perceptual
    with pytest.raises(NotImplementedError) as e:
        _build_perceptual({"perceptual_weight": 0.1}, None, torch.device("cpu"))
    assert "perceptual=" in str(e.value) and "perceptual_weights" in str(e.value)


def test_perceptual_weights_key_loads_a_local_state_dict(tmp_path):
    from fmdiff.nn.losses import VGGPerceptualLoss
    from fmdiff.pipelines.train.vae_lib import _build_perceptual
    torch.manual_seed(3)
    src = VGGPerceptualLoss()
    sd = {f"features.{k}": v for k, v in src.features.state_dict().items()}      # torchvision's vgg16 naming
    torch.save(sd, tmp_path / "vgg16.pt")
    got = _build_perceptual({"perceptual_weights": str(tmp_path / "vgg16.pt")}, None, torch.device("cpu"))
    assert got.resize == (224, 224)                                              # as the reference builds it
    for k, v in got.features.state_dict().items():
        assert torch.equal(v, sd[f"features.{k}"]), k
    given = VGGPerceptualLoss()
    assert _build_perceptual({"perceptual_weights": "unused.pt"}, given, torch.device("cpu")) is given
