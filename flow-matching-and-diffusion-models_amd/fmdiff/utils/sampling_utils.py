"""The evaluation CSV writers of the reference's ``src/utils/sampling_utils.py:284-339``: same file names,
header order, append-versus-overwrite behaviour and empty-rows behaviour.

* ``append_eval_metrics``: one summary row appended to ``<dir>/eval_metrics.csv``; the header (the row's keys in
  their order) is written only when the file does not exist yet.
* ``write_eval_metrics``: the same file overwritten with header + one row (an experiment directory's summary).
* ``append_per_image_eval_metrics``: ``<dir>/eval_metrics_per_image.csv`` overwritten with every row; the header
  is the union of the rows' keys in first-seen order, absent values are empty; no rows: an empty file is
  created unless one exists.
"""
from __future__ import annotations

import csv
from pathlib import Path
from typing import Dict, List

SUMMARY_NAME = "eval_metrics.csv"
PER_IMAGE_NAME = "eval_metrics_per_image.csv"


def _summary(root, row: Dict, mode: str) -> Path:
    path = Path(root) / SUMMARY_NAME
    path.parent.mkdir(parents=True, exist_ok=True)
    cells = {str(k): str(v) for k, v in row.items()}
    header = mode == "w" or not path.exists()
    with path.open(mode, newline="") as fh:
        w = csv.DictWriter(fh, fieldnames=list(cells))
        if header:
            w.writeheader()
        w.writerow(cells)
    return path


def append_eval_metrics(ckpt_dir, row: Dict) -> Path:
    return _summary(ckpt_dir, row, "a")


def write_eval_metrics(ckpt_dir, row: Dict) -> Path:
    return _summary(ckpt_dir, row, "w")


def append_per_image_eval_metrics(ckpt_dir, rows: List[Dict]) -> Path:
    path = Path(ckpt_dir) / PER_IMAGE_NAME
    path.parent.mkdir(parents=True, exist_ok=True)
    if not rows:
        if not path.exists():
            path.write_text("")
        return path
    names = list(dict.fromkeys(k for row in rows for k in row))
    with path.open("w", newline="") as fh:
        w = csv.DictWriter(fh, fieldnames=names)
        w.writeheader()
        for row in rows:
            w.writerow({k: row.get(k, "") for k in names})
    return path
