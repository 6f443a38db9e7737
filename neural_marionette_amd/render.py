"""The camera of the render path (NeuralMarionette.render_plates / render_frames, nm_render_bin / nm_render_draw): open3d's
PinholeCameraParameters as plain numbers, so that neither the library nor its users need open3d to draw what the reference's demo
scripts draw (vis_generation.py:171-190, vis_interpolation.py:177-185 read data/demo/source/source.json for it)."""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass, field
from typing import Sequence, Tuple

from . import _lib


def _identity() -> Tuple[Tuple[float, ...], ...]:
    return tuple(tuple(1.0 if r == c else 0.0 for c in range(4)) for r in range(4))


@dataclass(frozen=True)
class PinholeCamera:
    """extrinsic: the 4 x 4 world -> camera matrix, rows of rows (camera axes: x right, y down, z forward); fx, fy, cx, cy in pixels,
    open3d's convention - pixel (px, py) looks along ((px - cx) / fx, (py - cy) / fy, 1), so cx = width / 2 - 0.5 is the centre of the
    middle pixel; near: plates closer than this are not drawn (open3d's JSON has no such field)."""
    extrinsic: Tuple[Tuple[float, ...], ...] = field(default_factory=_identity)
    fx: float = 1.0
    fy: float = 1.0
    cx: float = 0.0
    cy: float = 0.0
    width: int = 1
    height: int = 1
    near: float = 1e-3

    def __post_init__(self):
        try:
            rows = tuple(tuple(float(v) for v in row) for row in self.extrinsic)
        except (TypeError, ValueError):
            rows = ()
        if len(rows) != 4 or any(len(r) != 4 for r in rows):
            raise ValueError("PinholeCamera: extrinsic must be a 4 x 4 matrix")
        object.__setattr__(self, "extrinsic", rows)
        for name in ("fx", "fy", "cx", "cy", "near"):
            object.__setattr__(self, name, float(getattr(self, name)))
        if int(self.width) != self.width or int(self.height) != self.height or self.width < 1 or self.height < 1:
            raise ValueError(f"PinholeCamera: width and height must be integers >= 1, got {self.width!r} x {self.height!r}")
        object.__setattr__(self, "width", int(self.width))
        object.__setattr__(self, "height", int(self.height))
        numbers = [v for r in rows for v in r] + [self.fx, self.fy, self.cx, self.cy, self.near]
        if not all(math.isfinite(v) for v in numbers):
            raise ValueError("PinholeCamera: every number must be finite")
        if self.fx == 0.0 or self.fy == 0.0 or not self.near > 0.0:
            raise ValueError(f"PinholeCamera: fx and fy must not be 0 and near must be > 0, got fx {self.fx}, fy {self.fy}, near {self.near}")

    @classmethod
    def from_open3d(cls, source, near: float = 1e-3) -> "PinholeCamera":
        """From open3d's PinholeCameraParameters JSON - a path, or the parsed dict.  Both of its matrices are column-major lists."""
        if isinstance(source, (str, bytes, os.PathLike)):
            with open(source) as f:
                source = json.load(f)
        try:
            e, intr = source["extrinsic"], source["intrinsic"]
            k, width, height = intr["intrinsic_matrix"], intr["width"], intr["height"]
            if len(e) != 16 or len(k) != 9:
                raise ValueError
            extrinsic = tuple(tuple(float(e[4 * c + r]) for c in range(4)) for r in range(4))
            fx, fy, cx, cy = float(k[0]), float(k[4]), float(k[6]), float(k[7])
        except (KeyError, TypeError, ValueError, IndexError):
            raise ValueError("PinholeCamera.from_open3d: not a PinholeCameraParameters JSON (extrinsic: 16 numbers, intrinsic: "
                             "width, height, intrinsic_matrix: 9 numbers)") from None
        return cls(extrinsic, fx, fy, cx, cy, width, height, near)

    def scaled(self, width: int, height: int) -> "PinholeCamera":
        """The same view at another resolution: fx' = fx W / W0 and cx' = (cx + 0.5) W / W0 - 0.5 (pixel centres sit at half-integers of
        the continuous image), the same along y."""
        sx, sy = width / self.width, height / self.height
        return PinholeCamera(self.extrinsic, self.fx * sx, self.fy * sy, (self.cx + 0.5) * sx - 0.5, (self.cy + 0.5) * sy - 0.5, width, height,
                             self.near)

    def flat_extrinsic(self) -> Sequence[float]:
        return [v for row in self.extrinsic for v in row]

    def c_struct(self) -> "_lib.NmCamera":
        """nm_camera of include/nm355.h (extrinsic row-major)"""
        cam = _lib.NmCamera()
        cam.extrinsic[:] = self.flat_extrinsic()
        cam.fx, cam.fy, cam.cx, cam.cy, cam.near, cam.width, cam.height = self.fx, self.fy, self.cx, self.cy, self.near, self.width, self.height
        return cam
