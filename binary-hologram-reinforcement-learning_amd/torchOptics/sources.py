"""torchOptics.sources -- illumination fields for the ``source=`` keyword of tt.simulate, tt.intensity
and tt.loss (reachable as ``tt.sources``).

Each function is computed in float64 numpy on pixel coordinates centred on the grid -- pixel (i, j) of
an H x W grid sits at y = (i - (H - 1) / 2) dy, x = (j - (W - 1) / 2) dx -- and returns a complex64
torch tensor on the CPU: [H, W] for one wavelength, [G, H, W] for a tuple of G wavelengths (one source
per colour group, the shape source= takes).  Sources multiply: an obliquely incident Gaussian beam is
``plane_wave(..) * gaussian(..)``; a lit disc is a product with a 0 / 1 array.

`shape` is (H, W); `dx` the pixel pitch in metres, one number or (dx, dy) as a tt.Tensor's meta carries
it; lengths (wl, waist, focal, center) in metres, angles in radians.
"""
from __future__ import annotations

import numpy as np
import torch

__all__ = ["plane_wave", "gaussian", "lens"]


def _grid(shape, dx):
    h, w = (int(v) for v in shape)
    if h < 1 or w < 1:
        raise ValueError(f"shape must be (H, W) with H, W >= 1, got {shape!r}")
    px, py = (float(dx), float(dx)) if np.isscalar(dx) else (float(dx[0]), float(dx[1]))
    y = (np.arange(h, dtype=np.float64) - (h - 1) / 2.0) * py
    x = (np.arange(w, dtype=np.float64) - (w - 1) / 2.0) * px
    return np.meshgrid(y, x, indexing="ij")


def _per_wavelength(wl, one):
    """one(wavelength) -> [H, W] complex128; a tuple of wavelengths stacks to [G, H, W]"""
    if isinstance(wl, (tuple, list)):
        out = np.stack([one(float(v)) for v in wl])
    else:
        out = one(float(wl))
    return torch.from_numpy(out.astype(np.complex64))


def plane_wave(shape, dx, wl, angle=(0.0, 0.0)) -> torch.Tensor:
    """exp(2 pi i (x sin ax + y sin ay) / wl): a unit plane wave incident at the angles (ax, ay) to the
    axis in the x and y directions (an obliquely lit DMD).  angle (0, 0) is 1 everywhere."""
    y, x = _grid(shape, dx)
    ax, ay = (float(v) for v in angle)
    return _per_wavelength(wl, lambda lam: np.exp(2j * np.pi * (x * np.sin(ax) + y * np.sin(ay)) / lam))


def gaussian(shape, dx, waist, center=(0.0, 0.0), wl=None) -> torch.Tensor:
    """exp(-r^2 / waist^2), r the distance from center = (cx, cy): the amplitude of a Gaussian beam at its
    waist, 1 at the centre and 1 / e at r = waist.  It does not depend on the wavelength; wl = a tuple of G
    wavelengths only repeats it to [G, H, W]."""
    y, x = _grid(shape, dx)
    cx, cy = (float(v) for v in center)
    a = np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / float(waist) ** 2).astype(np.complex128)
    return _per_wavelength(0.0 if wl is None else wl, lambda lam: a)


def lens(shape, dx, wl, focal) -> torch.Tensor:
    """exp(-i pi r^2 / (wl focal)): the paraxial phase of a thin lens of focal length `focal`, a reference
    wave converging to the axis at that distance (focal < 0: diverging).  Modulus 1, 1 at the centre."""
    y, x = _grid(shape, dx)
    r2 = x ** 2 + y ** 2
    return _per_wavelength(wl, lambda lam: np.exp(-1j * np.pi * r2 / (lam * float(focal))))
