"""Split-K planning of the weight gradients (csrc/wgrad.hip, csrc/wgrad_halo.hip): pure shape arithmetic, no
library and no device, so the rules can be tested on any host.

A weight gradient reduces over the pixels; with few output tiles the pixel range is split over workgroups and
every split stores an fp32 partial slab of the whole dW that a combine launch reads back.  Alone, a problem needs
enough splits to fill the chip, whatever its size -- about one 295 KB slab tile per CU per launch.  The jobs of
one UNet level that run on the same kernel instance can share a launch instead (fmd_wgrad_group): together they
still fill the chip, but each needs only 1/G of the splits, so the launch writes one chip's worth of slab for G
problems instead of one.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence, Tuple

GROUP_MAX = 16   # FMD_WGRAD_GROUP_MAX (include/fmdiff.h)


@dataclass(frozen=True)
class Shape:
    """One weight-gradient problem: dW[K][C][taps] over N x (Do x) Ho x Wo output pixels."""
    N: int
    Ho: int
    Wo: int
    K: int
    C: int
    ks: int = 3
    stride: int = 1
    halo: bool = True    # runs on the halo kernel (ops.wgrad_halo_eligible)
    pro: int = 0         # halo prologue form: 0 raw, 1 GroupNorm affine, 2 affine + SiLU
    Do: int = 0          # 3-D: output depth

    @property
    def taps(self) -> int:
        return self.ks * self.ks * (self.ks if self.Do else 1)

    @property
    def pixels(self) -> int:
        return self.N * max(self.Do, 1) * self.Ho * self.Wo

    @property
    def grid(self) -> Tuple[int, int, int, int]:
        return (self.N, self.Do, self.Ho, self.Wo)

    @property
    def key(self) -> tuple:
        """Kernel instance: one grouped launch holds jobs of one key."""
        return ("halo", self.pro, self.stride == 2) if self.halo else ("generic",)

    # ---- halo kernel: workgroup = (128 couts, 64-cin chunk [x depth tap | x stride-2 plane], tile split)
    @property
    def halo_tiles(self) -> int:
        return self.N * max(self.Do, 1) * (self.Ho // 8) * (self.Wo // 16)

    @property
    def halo_base(self) -> int:
        return (self.K // 128) * (self.C // 64) * (3 if self.Do else 1) * (4 if self.stride == 2 else 1)

    # ---- generic kernel: workgroup = (128 couts, 128 columns of a tap | of the flattened (tap, cin) pairs, split)
    @property
    def generic_tiles(self) -> int:
        T = self.taps
        cols = -(-(T * self.C) // 128) if T > 1 and self.C < 128 else -(-self.C // 128) * T
        return -(-self.K // 128) * cols

    @property
    def steps(self) -> int:
        return -(-self.pixels // 32)


def slab_floats(s: Shape, splits: int) -> int:
    """fmd_wgrad_workspace: the partial dW slabs and the partial db rows."""
    return splits * s.K * s.taps * s.C + splits * s.K


def halo_splits(s: Shape, target: int, slab_mb: int) -> int:
    """A halo job alone: enough tile splits for ``target`` workgroups, slabs capped at ``slab_mb``."""
    cap = (slab_mb << 20) // (s.K * s.C * 4 * s.taps)
    return max(1, min(s.halo_tiles, -(-target // s.halo_base), cap))


def generic_splits(s: Shape, num_cu: int, min_steps: int, cu_mult: int, slab_mb: int, tiles: int = 0) -> int:
    """A generic job alone (``tiles``: the total of its group instead of its own): up to ``cu_mult`` workgroups per
    CU, at least ``min_steps`` 32-pixel steps per split, slabs capped at ``slab_mb``."""
    cap = max(256, min(1024, (slab_mb << 20) // (s.K * s.C * s.taps * 4)))
    return max(1, min(s.steps // min_steps, -(-cu_mult * num_cu // (tiles or s.generic_tiles)), cap))


def single_splits(s: Shape, *, num_cu: int, halo_wg: int, slab_mb: int, gen_slab_mb: int, min_steps: int,
                  cu_mult: int) -> int:
    if s.halo:
        return halo_splits(s, halo_wg, slab_mb)
    return generic_splits(s, num_cu, min_steps, cu_mult, gen_slab_mb)


def _trim(units: int, splits: int) -> int:
    """The splits that own work when ``units`` (tiles, steps) are dealt ceil(units / splits) each."""
    return -(-units // -(-units // splits))


def plan_groups(jobs: Sequence[Shape], *, num_cu: int, halo_wg: int, slab_mb: int, gen_slab_mb: int, min_steps: int,
                cu_mult: int, cap: int = GROUP_MAX) -> List[Tuple[List[int], int]]:
    """Cut ``jobs`` (one key, one output grid, in issue order) into launches: [(job indices, splits)].

    Halo: the jobs of a level have the same pixel tiles and a workgroup's time is its tiles per split, so every
    job of a launch gets the same splits = floor(target / sum of base workgroups), within [1, tiles] and the slab
    cap.  Where the bases alone exceed one round of ``halo_wg`` workgroups the group is cut, so each launch is one
    whole round at splits >= 1 rather than a round and a fraction.
    Generic: the single-job rule on the group's total tiles (at the 8^2 level: 1 split, no slab duplication)."""
    if not jobs:
        return []
    if len({j.key for j in jobs}) != 1 or len({j.grid for j in jobs}) != 1:
        raise ValueError("a weight-gradient group holds jobs of one kernel instance and one output grid")
    out: List[Tuple[List[int], int]] = []
    if jobs[0].halo:
        cur: List[int] = []
        base = 0

        def close():
            slab = sum(jobs[i].K * jobs[i].C * 4 * jobs[i].taps for i in cur)
            tiles = min(jobs[i].halo_tiles for i in cur)
            out.append((list(cur), _trim(tiles, max(1, min(tiles, halo_wg // base, (slab_mb << 20) // slab)))))

        for i, j in enumerate(jobs):
            if cur and (len(cur) >= cap or base + j.halo_base > halo_wg):
                close()
                cur, base = [], 0
            cur.append(i)
            base += j.halo_base
        close()
        return out
    for lo in range(0, len(jobs), cap):
        idx = list(range(lo, min(len(jobs), lo + cap)))
        tiles = sum(jobs[i].generic_tiles for i in idx)
        s = min(generic_splits(jobs[i], num_cu, min_steps, cu_mult, gen_slab_mb, tiles) for i in idx)
        out.append((idx, _trim(jobs[idx[0]].steps, s)))
    return out


def slab_bytes(jobs: Sequence[Shape], splits: Sequence[int]) -> int:
    """Bytes of partial slab one pass over the jobs writes (the combine reads the same again)."""
    return 4 * sum(slab_floats(j, s) for j, s in zip(jobs, splits))
