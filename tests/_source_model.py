"""The float64 model of illumination fields (hbx_source_field / hbx_evaluate_source /
hbx_backward_source), built from the oracle's O.propagate and OpticsConfig.transfer.

    forward   u64 = s64 * f64(x)                      f the leaf kind's map, s the source of the plane's group
              F   = O.propagate(u64, h)
    adjoint   g   = O.propagate(v, conj h)            v the values (times scale * weight where given)
              g'  = conj(s64) g
              complex g', real Re g', phase and L-level pi (Im g' cos pi q - Re g' sin pi q),
              thresholded vb ste(x) Re g' with both surrogates

Every array is float64 / complex128 of the float32 / complex64 inputs, so no input rounding enters a
comparison.  The L-level kind starts from the materialised q (hbx.quantize_phase's samples): the model
does not restate the quantizer.  Shapes: x, q, v [G * Q, N, N]; source [G, N, N]; weight [G, N, N]."""
import numpy as np

from oracle import hbx_oracle as O

KINDS = ("complex", "real", "threshold", "phase", "levels")


def leaf_field(kind, x, q=None, tau=0.5, va=0.0, vb=1.0):
    """f64(x) of one leaf kind, complex128: x as it is (complex, real), va + vb [x >= tau] (threshold; NaN
    compares false), exp(i pi x) (phase), exp(i pi q) (levels: q the materialised quantized samples)"""
    if kind == "complex":
        return x.astype(np.complex128)
    if kind == "real":
        return x.astype(np.float64).astype(np.complex128)
    if kind == "threshold":
        return (va + vb * (x.astype(np.float64) >= tau)).astype(np.complex128)
    if kind == "phase":
        return np.exp(1j * np.pi * x.astype(np.float64))
    if kind == "levels":
        return np.exp(1j * np.pi * q.astype(np.float64))
    raise ValueError(kind)


def per_plane(a, planes_per_group):
    """[G, N, N] -> [G * Q, N, N]: a group's image repeated for each of its planes"""
    return np.repeat(a, planes_per_group, axis=0)


def sourced(kind, x, source, q=None, tau=0.5, va=0.0, vb=1.0):
    """u64 = s64 * f64(x), [G * Q, N, N] complex128"""
    f = leaf_field(kind, x, q, tau, va, vb)
    return per_plane(source.astype(np.complex128), f.shape[0] // source.shape[0]) * f


def forward(ocfg, u):
    """F = A u per colour group: u [G * Q, N, N] complex128 -> the same shape"""
    g = ocfg.groups
    qn = u.shape[0] // g
    return np.concatenate([O.propagate(u[k * qn:(k + 1) * qn], ocfg.transfer(k)) for k in range(g)])


def adjoint(ocfg, v):
    """A^H v per colour group (the plan for -z: conj H(z) = H(-z))"""
    g = ocfg.groups
    qn = v.shape[0] // g
    return np.concatenate([O.propagate(v[k * qn:(k + 1) * qn], np.conj(ocfg.transfer(k))) for k in range(g)])


def intensity(ocfg, field):
    """the plane mean of |F|^2 per group, [G, N, N]"""
    g = ocfg.groups
    return np.mean(np.abs(field.reshape((g, field.shape[0] // g) + field.shape[1:])) ** 2, axis=1)


def ste(x, surrogate, p0, p1):
    """the surrogate derivative s(x): 'window' 1 on p0 <= x <= p1 else 0; 'sigmoid' k sg (1 - sg) with
    sg = sigmoid(k (x - p0)), k = p1"""
    x = x.astype(np.float64)
    if surrogate == "window":
        return ((x >= p0) & (x <= p1)).astype(np.float64)
    sg = 1.0 / (1.0 + np.exp(-p1 * (x - p0)))
    return p1 * sg * (1.0 - sg)


def leaf_gradient(kind, gp, x=None, q=None, vb=1.0, surrogate="window", p0=-np.inf, p1=np.inf):
    """the leaf's gradient from g' = conj(s) g"""
    if kind == "complex":
        return gp
    if kind == "real":
        return gp.real
    if kind in ("phase", "levels"):
        a = (x if kind == "phase" else q).astype(np.float64)
        return np.pi * (gp.imag * np.cos(np.pi * a) - gp.real * np.sin(np.pi * a))
    if kind == "threshold":
        return vb * ste(x, surrogate, p0, p1) * gp.real
    raise ValueError(kind)


def backward(ocfg, kind, v, source, weight=None, scale=1.0, **leaf):
    """(g' [G * Q, N, N] complex128, the leaf's gradient): v complex [G * Q, N, N], optionally times
    scale * weight [G, N, N] of its group"""
    v = v.astype(np.complex128)
    qn = v.shape[0] // ocfg.groups
    if weight is not None:
        v = v * (scale * per_plane(weight.astype(np.float64), qn))
    gp = np.conj(per_plane(source.astype(np.complex128), qn)) * adjoint(ocfg, v)
    return gp, leaf_gradient(kind, gp, **leaf)


def weighted_energy(ocfg, kind, x, source, w):
    """L = sum w |A(s f(x))|^2 (w [G * Q, N, N] real), and its gradient with respect to the leaf by the
    model above: dL/du = A^H(2 w F), then conj(s) and the leaf's formula.  For the self-check against
    finite differences."""
    field = forward(ocfg, sourced(kind, x, source))
    loss = float(np.sum(w * np.abs(field) ** 2))
    qn = field.shape[0] // ocfg.groups
    gp = np.conj(per_plane(source.astype(np.complex128), qn)) * adjoint(ocfg, 2.0 * w * field)
    return loss, leaf_gradient(kind, gp, x=x)
