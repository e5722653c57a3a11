"""The VGG perceptual loss of VAE training (reference ``src/nn/losses/vae.py:22-72``) on the HIP engine
(``fmdiff.runtime.perc_engine``, ``csrc/perceptual.hip``).

``VGGPerceptualLoss`` holds a frozen ``features`` stack of ``Conv2d(3x3, stride 1, padding 1)``, ``ReLU`` and
``MaxPool2d(2, 2)`` and computes ``sum_l w_l mean |f_l(rec) - f_l(target)|`` over the outputs of the tapped layers
(3, 8, 15, 22: relu1_2, relu2_2, relu3_3, relu4_3 of VGG16).  As in the reference a 1-channel image is repeated to
three channels, there is no ImageNet normalisation, and ``resize`` interpolates both images bilinearly
(``align_corners=False``) first.

No weights ship with the package: the default stack has the VGG16 ``features[:23]`` topology with torch's default
initialisation, and ``load_vgg_state_dict`` takes a torchvision ``vgg16`` state dict.  Unlike the
reference, nothing here returns 0 when something is missing: a loss term that vanishes without saying so is a bug.
Inputs are ROCm device tensors; there is no CPU path."""
from __future__ import annotations

from typing import Iterable, List, NamedTuple, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn

__all__ = ["VGGPerceptualLoss", "VGG16_WIDTHS"]

# VGG16 features[:23]: conv widths, "M" a 2x2 max pool
VGG16_WIDTHS = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512)


class TapSpec(NamedTuple):
    """One ``conv -> ReLU [-> pool]`` step of the walker."""
    conv: nn.Conv2d
    tap: Optional[int]   # which term of the loss the ReLU's output feeds (ascending), or None
    weight: float        # that term's weight
    pool: bool           # a 2x2 max pool follows (and something follows the pool)


def build_features(widths: Sequence = VGG16_WIDTHS, in_channels: int = 3) -> nn.Sequential:
    """``Conv2d(3x3, padding 1) -> ReLU`` per width and ``MaxPool2d(2, 2)`` per "M", torch's default initialisation."""
    mods: List[nn.Module] = []
    cin = in_channels
    for w in widths:
        if w == "M":
            mods.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            mods += [nn.Conv2d(cin, int(w), kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = int(w)
    return nn.Sequential(*mods)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class VGGPerceptualLoss(nn.Module):
    def __init__(self, features: Optional[nn.Sequential] = None, *, resize: Union[bool, int, Tuple[int, int]] = False,
                 layers: Iterable[int] = (3, 8, 15, 22), layer_weights: Iterable[float] = (1.0, 1.0, 1.0, 1.0)) -> None:
        super().__init__()
        self.features = build_features() if features is None else features
        if not isinstance(self.features, nn.Sequential):
            raise NotImplementedError("VGGPerceptualLoss: features must be an nn.Sequential of Conv2d, ReLU, MaxPool2d")
        if resize is True:
            self.resize: Optional[Tuple[int, int]] = (224, 224)   # the reference's
        elif resize is False or resize is None:
            self.resize = None
        else:
            hw = tuple(int(v) for v in _pair(resize))
            if len(hw) != 2 or hw[0] < 1 or hw[1] < 1:
                raise ValueError(f"VGGPerceptualLoss: resize must be a bool, a positive int or (h, w), got {resize!r}")
            self.resize = hw
        self.layers = tuple(sorted({int(v) for v in layers}))
        if not self.layers:
            raise ValueError("VGGPerceptualLoss: no layers to tap")
        if self.layers[0] < 0 or self.layers[-1] >= len(self.features):
            raise ValueError(f"VGGPerceptualLoss: layers {self.layers} reach past the {len(self.features)} modules of "
                             "features")
        wts = [float(v) for v in layer_weights]
        # a shorter list is filled with 1.0, as the reference's next(weight_iter, 1.0); weights follow ascending layers
        self.layer_weights = tuple((wts + [1.0] * len(self.layers))[:len(self.layers)])
        for p in self.features.parameters():
            p.requires_grad_(False)
        self.layer_specs()                    # refuses a stack the walker cannot run
        self.layer_values: Optional[torch.Tensor] = None   # the per-tap means of the last call (device, diagnostics)

    # ------------------------------------------------------------------ the Sequential read back as walker layers
    def layer_specs(self) -> List[TapSpec]:
        what = type(self).__name__
        mods = list(self.features)
        taps = {layer: k for k, layer in enumerate(self.layers)}
        for layer in self.layers:
            if not isinstance(mods[layer], nn.ReLU):
                raise NotImplementedError(f"{what}: tapped layer {layer} is a {type(mods[layer]).__name__}, not a ReLU")
        specs: List[TapSpec] = []
        i, end = 0, self.layers[-1]
        while i <= end:
            conv = mods[i]
            if not isinstance(conv, nn.Conv2d) or i + 1 >= len(mods) or not isinstance(mods[i + 1], nn.ReLU):
                raise NotImplementedError(f"{what}: module {i} ({type(conv).__name__}): the stack is Conv2d -> ReLU "
                                          "[-> MaxPool2d]")
            if (conv.kernel_size != (3, 3) or conv.stride != (1, 1) or conv.padding != (1, 1) or
                    conv.dilation != (1, 1) or conv.groups != 1 or conv.bias is None or conv.padding_mode != "zeros"):
                raise NotImplementedError(f"{what}: conv {i}: 3x3, stride 1, zero padding 1 and a bias only")
            cin = 3 if not specs else specs[-1].conv.out_channels
            if conv.in_channels != cin:
                raise NotImplementedError(f"{what}: conv {i} reads {conv.in_channels} channels, its input has {cin}")
            tap = taps.get(i + 1)
            i += 2
            pool = False
            if i <= end and isinstance(mods[i], nn.MaxPool2d):
                p = mods[i]
                if tap is None:
                    raise NotImplementedError(f"{what}: the pool at {i} does not follow a tapped ReLU (the pool is fused "
                                              "into the tap kernel)")
                if (_pair(p.kernel_size) != (2, 2) or _pair(p.stride) != (2, 2) or _pair(p.padding) != (0, 0) or
                        _pair(p.dilation) != (1, 1) or p.ceil_mode or p.return_indices):
                    raise NotImplementedError(f"{what}: pool {i}: MaxPool2d(2, 2) only")
                pool = True
                i += 1
            specs.append(TapSpec(conv, tap, self.layer_weights[tap] if tap is not None else 0.0, pool))
        return specs

    def feature_sizes(self, hw: Tuple[int, int]) -> List[Tuple[int, int]]:
        """(H, W) of every conv's output; ValueError if the input is too small for the stack."""
        h, w = (int(v) for v in hw)
        sizes = []
        for spec in self.layer_specs():
            if h < 1 or w < 1:
                raise ValueError(f"{type(self).__name__}: a {hw[0]}x{hw[1]} input is too small for the stack (conv "
                                 f"{len(sizes)} would read {h}x{w})")
            sizes.append((h, w))
            if spec.pool:
                h, w = h // 2, w // 2
        return sizes

    # ------------------------------------------------------------------ weights
    def conv_indices(self) -> List[int]:
        return [i for i, m in enumerate(self.features) if isinstance(m, nn.Conv2d)]

    def load_vgg_state_dict(self, sd) -> None:
        """Load the conv weights from a torchvision ``vgg16`` state dict (``features.<i>.weight``) or from that of its
        ``.features`` (``<i>.weight``).  The classifier and the layers this stack does not hold are ignored; a missing
        tensor is a KeyError that names it."""
        with torch.no_grad():
            for i in self.conv_indices():
                for name, dst in (("weight", self.features[i].weight), ("bias", self.features[i].bias)):
                    key = f"features.{i}.{name}"
                    src = sd[key] if key in sd else sd.get(f"{i}.{name}")
                    if src is None:
                        raise KeyError(f"load_vgg_state_dict: '{key}' (or '{i}.{name}') is missing")
                    if tuple(src.shape) != tuple(dst.shape):
                        raise ValueError(f"load_vgg_state_dict: '{key}' is {tuple(src.shape)}, expected "
                                         f"{tuple(dst.shape)}")
                    dst.copy_(src)
        self.invalidate_weights()

    def invalidate_weights(self) -> None:
        """After the weights were written through raw pointers: re-derive the bf16 kernel layouts."""
        eng = getattr(self, "_fmd_perc_engine", None)
        if eng is not None:
            eng.invalidate_weights()

    # ------------------------------------------------------------------ forward
    def forward(self, recon: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """``recon``, ``target``: images ``[N, 1 or 3, H, W]`` fp32 on the device.  Returns the loss, a device fp32
        scalar connected to ``recon`` by autograd (the target and the stack receive no gradient)."""
        return self.forward_image(recon, "identity", target)

    def forward_image(self, raw: torch.Tensor, image_map: str, target: torch.Tensor) -> torch.Tensor:
        """``forward`` of ``image_map(raw)`` with the map fused into the staging: "identity", "clamp"
        (``(clamp(raw, -1, 1) + 1) / 2``) or "sigmoid", the reference's ``raw_output_to_image``."""
        from ...runtime.perc_engine import perc_apply
        loss, values = perc_apply(self, raw, target, image_map)
        self.layer_values = values.detach()
        return loss
