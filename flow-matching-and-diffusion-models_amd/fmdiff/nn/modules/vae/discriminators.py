"""GAN discriminators of VAE training (reference ``src/nn/modules/vae/discriminators.py`` and the
``PatchDiscriminator`` stack of ``src/nn/losses/vae.py``), state_dict-compatible with the reference.

Both classes are an ``nn.Sequential`` named ``model`` of parameter holders (``ConvND``, ``nn.BatchNorm2d``,
``nn.LeakyReLU``) built from one layer table; ``forward`` runs the table on the HIP engine
(``fmdiff.runtime.disc_engine``): one autograd node from the logits to the input and the parameters.  There is no CPU
path, and only ``spatial_dims=2`` (all of VAE training here is 2-D).
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from ...ops.convolution import ConvND
from ...params import Conv

__all__ = ["MagvitDiscriminatorND", "MagvitDiscriminator", "PatchGANDiscriminatorND"]

SLOPE = 0.2


class LayerSpec(NamedTuple):
    """One ``conv -> [BatchNorm] -> [LeakyReLU]`` layer of the walker."""
    conv: Conv
    norm: Optional[nn.BatchNorm2d]
    slope: Optional[float]   # None: the output layer (no activation)
    ks: int
    stride: int
    pad: int


# (output width as a multiple of base_channels (0: the single logit), kernel, stride, padding, norm, activation)
MAGVIT_TABLE = ((1, 4, 2, 1, False, True), (2, 4, 2, 1, True, True), (4, 4, 2, 1, True, True),
                (8, 4, 1, 1, True, True), (0, 4, 1, 0, False, False))
PATCHGAN_TABLE = ((1, 4, 2, 1, False, True), (2, 4, 2, 1, True, True), (4, 4, 2, 1, True, True),
                  (8, 4, 2, 1, True, True), (0, 3, 1, 1, False, False))


class _TableDiscriminator(nn.Module):
    TABLE: Sequence[Tuple] = ()

    def __init__(self, in_channels: int, base_channels: int, spatial_dims: int) -> None:
        super().__init__()
        if spatial_dims not in (1, 2, 3):
            raise ValueError("spatial_dims must be 1, 2 or 3")
        if spatial_dims != 2:
            raise NotImplementedError(f"{type(self).__name__}: spatial_dims=2 only (VAE training on the HIP engine "
                                      f"is 2-D), got {spatial_dims}")
        self.in_channels, self.base_channels, self.spatial_dims = in_channels, base_channels, spatial_dims
        mods: List[nn.Module] = []
        cin = in_channels
        for mult, ks, stride, pad, norm, act in self.TABLE:
            cout = base_channels * mult if mult else 1
            mods.append(ConvND(spatial_dims, cin, cout, ks, stride, pad))
            if norm:
                mods.append(nn.BatchNorm2d(cout))
            if act:
                mods.append(nn.LeakyReLU(SLOPE, inplace=True))
            cin = cout
        self.model = nn.Sequential(*mods)

    def layer_specs(self) -> List[LayerSpec]:
        """The Sequential read back as walker layers (so a ``model`` edited by hand is refused, not misread)."""
        specs, mods, i = [], list(self.model), 0
        while i < len(mods):
            if not isinstance(mods[i], ConvND):
                raise NotImplementedError(f"{type(self).__name__}: unexpected layer {type(mods[i]).__name__}")
            conv = mods[i].conv
            i += 1
            norm = slope = None
            if i < len(mods) and isinstance(mods[i], nn.BatchNorm2d):
                norm = mods[i]
                if not (norm.affine and norm.track_running_stats) or norm.momentum is None:
                    raise NotImplementedError("BatchNorm2d: affine, tracked statistics and a fixed momentum")
                i += 1
            if i < len(mods) and isinstance(mods[i], nn.LeakyReLU):
                slope = float(mods[i].negative_slope)
                i += 1
            ks, stride, pad = conv.kernel_size[0], conv.stride[0], conv.padding[0]
            if conv.kernel_size != (ks, ks) or conv.stride != (stride, stride) or conv.padding != (pad, pad):
                raise NotImplementedError(f"conv geometry {conv.kernel_size}/{conv.stride}/{conv.padding}")
            specs.append(LayerSpec(conv, norm, slope, ks, stride, pad))
        if not specs or specs[-1].slope is not None or specs[-1].norm is not None or any(
                s.slope is None for s in specs[:-1]):
            raise NotImplementedError(f"{type(self).__name__}: activations on every layer but a plain output conv")
        return specs

    def output_sizes(self, hw: Tuple[int, int]) -> List[Tuple[int, int]]:
        """(H, W) of the input and after every conv; ValueError if the input is too small for the stack."""
        sizes = [tuple(int(v) for v in hw)]
        for mult, ks, stride, pad, _, _ in self.TABLE:
            h, w = ((v + 2 * pad - ks) // stride + 1 for v in sizes[-1])
            if h < 1 or w < 1:
                raise ValueError(f"{type(self).__name__}: a {sizes[0][0]}x{sizes[0][1]} input is too small (layer "
                                 f"{len(sizes)} would be {h}x{w})")
            sizes.append((h, w))
        return sizes

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """Image batch ``[N, C, H, W]`` fp32 on the device -> logits ``[N, 1, h, w]`` fp32."""
        return self.forward_image(x, "identity")

    def forward_image(self, raw: torch.Tensor, image_map: str = "identity", param_grads: bool = True) -> torch.Tensor:
        """``forward`` of ``image_map(raw)`` with the map fused into the input staging: "identity", "clamp"
        (``(clamp(raw, -1, 1) + 1) / 2``) or "sigmoid", the reference's ``raw_output_to_image``.  ``param_grads``
        False: the backward of this call leaves the discriminator's ``.grad`` alone."""
        from ....runtime.disc_engine import disc_apply
        return disc_apply(self, raw, image_map, param_grads)

    def invalidate_weights(self) -> None:
        """After an optimizer that wrote the parameters through raw pointers: re-derive the bf16 kernel layouts."""
        from ....runtime.disc_engine import get_disc_engine
        get_disc_engine(self).invalidate_weights()


class MagvitDiscriminatorND(_TableDiscriminator):
    """MAGVIT-style discriminator: three stride-2 and two stride-1 4x4 convs, widths ch, 2ch, 4ch, 8ch, 1."""
    TABLE = MAGVIT_TABLE

    def __init__(self, in_channels: int = 3, base_channels: int = 64, spatial_dims: int = 2) -> None:
        super().__init__(in_channels, base_channels, spatial_dims)


class MagvitDiscriminator(MagvitDiscriminatorND):
    """The 2-D alias."""

    def __init__(self, in_channels: int = 3, base_channels: int = 64) -> None:
        super().__init__(in_channels=in_channels, base_channels=base_channels, spatial_dims=2)


class PatchGANDiscriminatorND(_TableDiscriminator):
    """The reference's ``PatchDiscriminator`` stack: four stride-2 4x4 convs and a 3x3 conv to one logit."""
    TABLE = PATCHGAN_TABLE

    def __init__(self, in_channels: int = 1, base_channels: int = 64, spatial_dims: int = 2) -> None:
        super().__init__(in_channels, base_channels, spatial_dims)
