"""Cone specification types, mirroring the reference's user-facing cone API
(`/root/reference/src/cones/cone_api.jl:18-55`): a problem's cone list is a sequence of
`ZeroConeT(dim)`, `NonnegativeConeT(dim)`, `SecondOrderConeT(dim)`, `PSDTriangleConeT(k)`,
`ExponentialConeT()`, `PowerConeT(alpha)`, `GenPowerConeT(alpha, dim2)`.

`PSDTriangleConeT(k)` takes the matrix side length k; the cone then has k(k+1)/2 rows
(`cone_types.jl:171-186`).  Kind codes are the ones `include/hipkkt.h` uses.
"""
from dataclasses import dataclass

KIND_ZERO, KIND_NN, KIND_SOC, KIND_PSD, KIND_EXP, KIND_POW, KIND_GENPOW = 0, 1, 2, 3, 4, 5, 6

# cone_types.jl:101 -- second-order cones larger than this use the sparse expansion
SOC_NO_EXPANSION_MAX_SIZE = 4


@dataclass(frozen=True)
class _ConeT:
    dim: int

    @property
    def numel(self) -> int:
        return self.dim


class ZeroConeT(_ConeT):
    kind = KIND_ZERO


class NonnegativeConeT(_ConeT):
    kind = KIND_NN


class SecondOrderConeT(_ConeT):
    kind = KIND_SOC



class PSDTriangleConeT(_ConeT):
    kind = KIND_PSD

    @property
    def numel(self) -> int:
        return self.dim * (self.dim + 1) // 2


@dataclass(frozen=True)
class ExponentialConeT(_ConeT):
    """{(x, y, z): y exp(x/y) <= z, y > 0}; always three rows (cone_types.jl)."""
    dim: int = 3
    kind = KIND_EXP


@dataclass(frozen=True)
class PowerConeT(_ConeT):
    """{(x, y, z): x^alpha y^(1-alpha) >= |z|, x, y >= 0}; always three rows, 0 < alpha < 1."""
    alpha: float = 0.5
    dim: int = 3
    kind = KIND_POW

    def __init__(self, alpha):
        object.__setattr__(self, "alpha", float(alpha))
        object.__setattr__(self, "dim", 3)


@dataclass(frozen=True)
class GenPowerConeT(_ConeT):
    """{(u, w): prod_i u_i^alpha_i >= ||w||, u >= 0} with u of length len(alpha) and w of length dim2;
    dim = len(alpha) + dim2.  Validated as the reference's constructor does (cone_api.jl:37-47): every alpha
    positive (and finite), |sum(alpha) - 1| <= eps len(alpha) / 2; and both blocks non-empty."""
    alpha: tuple = ()
    dim2: int = 1
    dim: int = 0
    kind = KIND_GENPOW

    def __init__(self, alpha, dim2):
        import math
        alpha = tuple(float(a) for a in alpha)
        dim2 = int(dim2)
        if len(alpha) < 1 or dim2 < 1:
            raise ValueError("GenPowerConeT needs at least one alpha and dim2 >= 1")
        if not all(a > 0.0 and math.isfinite(a) for a in alpha):
            raise ValueError("GenPowerConeT: every alpha must be positive and finite")
        total = 0.0
        for a in alpha:
            total += a
        if not abs(total - 1.0) <= 2.220446049250313e-16 * len(alpha) / 2:
            raise ValueError("GenPowerConeT: the alphas must sum to 1")
        object.__setattr__(self, "alpha", alpha)
        object.__setattr__(self, "dim2", dim2)
        object.__setattr__(self, "dim", len(alpha) + dim2)

    @property
    def dim1(self) -> int:
        return len(self.alpha)


def cones_new_collapsed(cones):
    """Merge runs of nonnegative cones (and 1-D second-order / PSD cones, which are
    nonnegative cones) into one, and drop empty cones, as the reference does before the
    KKT system sees the list (`cone_api.jl:96-153`)."""
    def collapsible(c):
        return isinstance(c, NonnegativeConeT) or (
            isinstance(c, (SecondOrderConeT, PSDTriangleConeT)) and c.dim == 1)

    out = []
    run = None  # total dim of the nonnegative run being collapsed
    for c in cones:
        if c.numel == 0:
            continue
        if collapsible(c):
            run = (run or 0) + c.numel
            continue
        if run is not None:
            out.append(NonnegativeConeT(run))
            run = None
        out.append(c)
    if run is not None:
        out.append(NonnegativeConeT(run))
    return out


def cone_kinds_dims(cones):
    import numpy as np
    kinds = np.array([c.kind for c in cones], dtype=np.int32)
    dims = np.array([c.dim for c in cones], dtype=np.int64)
    return kinds, dims


def cone_params(cones):
    """One double per cone for hipkkt_kkt_create_ex: alpha of a power cone, 0 otherwise."""
    import numpy as np
    return np.array([c.alpha if c.kind == KIND_POW else 0.0 for c in cones], dtype=np.float64)


def cone_param_ptr_vals(cones):
    """Ragged parameters for hipkkt_kkt_create_ex2: (ptr (ncones + 1 offsets, 0-based), vals) -- one alpha for a power
    cone, its dim1 alphas for a generalized power cone, nothing for every other kind."""
    import numpy as np
    ptr, vals = [0], []
    for c in cones:
        if c.kind == KIND_POW:
            vals.append(c.alpha)
        elif c.kind == KIND_GENPOW:
            vals.extend(c.alpha)
        ptr.append(len(vals))
    return np.array(ptr, dtype=np.int64), np.array(vals, dtype=np.float64)


def has_nonsymmetric(cones) -> bool:
    return any(c.kind in (KIND_EXP, KIND_POW, KIND_GENPOW) for c in cones)


def total_numel(cones) -> int:
    return sum(c.numel for c in cones)
