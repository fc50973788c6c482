"""Plain numpy restatement of Preprocess (filter off) and VoxelDownsample, for the tests only.

Written from the reference's text (core/Preprocessing.cpp:173-187 Preprocess, :44-84 VoxelDownsample, pipeline/sageICP.cpp:
97-101 Voxelize) in fp64, vectorised so that 200k rows take milliseconds.  VoxelDownsample emits in ARRIVAL order: group by
group, each group's survivors by input index (deviation D3, DESIGN.md: the reference itself emits tsl::robin_map bucket
order, which oracle.voxel_downsample reproduces in mode 1).

What the reference leaves undefined is refused here the way the product refuses it (include/sageicp.h): a row that reaches
VoxelDownsample with a non-finite label or coordinate (the cast to int is undefined), and a voxel index outside
[-2^19, 2^19) of a row whose label is listed: Refused, with .code the name of the product's error.

Every function takes variant=, which selects ONE deliberately wrong evaluation (VARIANTS).  tests/prepscenes.py uses it to
prove that a scene tells that wrong kernel from the right one.  A variant is never an expectation.

py_preprocess / py_voxel_downsample are the literal per-point loops (what tests/test_pipeline.py compares the device
against); tests/test_preprocess_host.py holds the vectorised functions to them row for row."""
import os
from fractions import Fraction

import numpy as np

# the association of the crop's 3-term squared norm (csrc/sageicp_types.h, SAGE_SQNORM3_CROP): the library and the
# oracle follow this variable, and so does this restatement.  2 (default): (x^2 + y^2) + z^2; 0: x^2 + (y^2 + z^2)
SQNORM3_ORDER = 0 if os.environ.get("SAGE_SQNORM3_ORDER", "2") == "0" else 2

KEY_LIMIT = 1 << 19         # voxel indices live in [-2^19, 2^19)

CROP_VARIANTS = ("assoc",       # the other association of the norm^2
                 "fma_full",    # every add of a product contracted: fma(z, z, fma(x, x, y*y)) / fma(x, x, fma(y, y, z*z))
                 "fma_outer",   # only the last add contracted: fma(z, z, x*x + y*y) / fma(x, x, y*y + z*z)
                 "max_le", "min_ge", "label_ge")     # <= / >= at the three thresholds
VDS_VARIANTS = ("recip",        # p * (1 / vs) instead of p / vs
                "fp32",         # the division in fp32
                "floor",        # floor instead of truncation toward zero
                "label_round",  # the label rounded to nearest instead of truncated
                "last_wins")    # the HIGHEST input index of a voxel survives
CHAIN_VARIANTS = ("stale_label",)   # level 0 looks the group up with the label as it was before zeroing
VARIANTS = CROP_VARIANTS + VDS_VARIANTS + CHAIN_VARIANTS


class Refused(ValueError):
    def __init__(self, code, why):
        super().__init__("%s: %s" % (code, why))
        self.code = code            # "ERR_INVALID" or "ERR_CAPACITY"


def _rows(frame):
    return np.ascontiguousarray(frame, dtype=np.float64).reshape(-1, 4)


def _fl(q):
    """the double nearest to the rational q (ties to even), Inf beyond the range"""
    try:
        return float(q)
    except OverflowError:
        return float("inf") if q > 0 else float("-inf")


def sqnorm3(xyz, variant=None):
    """x^2 + y^2 + z^2 per row as the crop evaluates it: three rounded products, two rounded adds in the association
    SQNORM3_ORDER selects; the fma variants round the contracted operations once (exact rationals)"""
    order = SQNORM3_ORDER
    if variant == "assoc":
        order = 0 if order == 2 else 2
    x, y, z = (np.ascontiguousarray(xyz[:, a], dtype=np.float64) for a in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        xx, yy, zz = x * x, y * y, z * z
        plain = (xx + yy) + zz if order == 2 else xx + (yy + zz)
    if variant not in ("fma_full", "fma_outer"):
        return plain
    out = plain.copy()
    fin = np.flatnonzero(np.isfinite(x) & np.isfinite(y) & np.isfinite(z))
    for i in fin.tolist():
        a, b, c = (x[i], y[i], z[i]) if order == 2 else (z[i], y[i], x[i])      # (a^2 + b^2) + c^2 in both orders
        bb = _fl(Fraction(b) * Fraction(b))
        inner = _fma(a, a, bb) if variant == "fma_full" else _fl(Fraction(a) * Fraction(a)) + bb
        out[i] = _fma(c, c, inner)
    return out


def _fma(a, b, c):
    """a * b + c rounded once"""
    return c if not np.isfinite(c) else _fl(Fraction(a) * Fraction(b) + Fraction(c))


def crop_norm(frame, variant=None):
    """point.head<3>().norm() per row (Preprocessing.cpp:176)"""
    with np.errstate(invalid="ignore"):
        return np.sqrt(sqnorm3(_rows(frame)[:, :3], variant))


def preprocess(frame, max_range, min_range, label_max_range, variant=None, return_index=False):
    """Preprocessing.cpp:173-187: rows with norm < max_range && norm > min_range, the label zeroed where
    norm > label_max_range, order preserved"""
    assert variant is None or variant in VARIANTS, variant
    f = _rows(frame)
    norm = crop_norm(f, variant)
    with np.errstate(invalid="ignore"):
        below = norm <= max_range if variant == "max_le" else norm < max_range
        above = norm >= min_range if variant == "min_ge" else norm > min_range
        far = norm >= label_max_range if variant == "label_ge" else norm > label_max_range
    idx = np.flatnonzero(below & above)
    out = f[idx].copy()
    out[far[idx], 3] = 0.0
    return (out, idx) if return_index else out


def _groups_of(label, voxel_labels):
    """the first group that lists the label, -1 where none does"""
    group = np.full(len(label), -1, dtype=np.int64)
    for g, listed in enumerate(voxel_labels):
        if len(listed):
            hit = (group < 0) & np.isin(label, np.asarray(listed, dtype=np.int64))
            group[hit] = g
    return group


def voxel_downsample(frame, voxel_labels, voxel_size, scale, variant=None, return_index=False, _lookup_labels=None):
    """Preprocessing.cpp:44-84 in arrival order: label = trunc toward zero; the first group that lists it (none: dropped);
    index = trunc(p / (size[g] * scale)) per axis, a true division; the lowest input index per (group, voxel) survives;
    emitted group-major, then by input index"""
    assert variant is None or variant in VARIANTS, variant
    f = _rows(frame)
    assert len(voxel_labels) == len(voxel_size) <= 8
    if not np.all(np.isfinite(f)):
        raise Refused("ERR_INVALID", "a label or a coordinate is not finite")
    lab = f[:, 3] if _lookup_labels is None else np.asarray(_lookup_labels, dtype=np.float64)
    assert np.all(np.abs(lab) <= 2.0 ** 30), "labels beyond int are undefined in the reference too"
    label = (np.rint(lab) if variant == "label_round" else np.trunc(lab)).astype(np.int64)
    group = _groups_of(label, voxel_labels)
    rows = np.flatnonzero(group >= 0)
    empty = (np.zeros((0, 4)), np.zeros(0, dtype=np.int64))
    if len(rows) == 0:
        return empty if return_index else empty[0]
    vs = (np.asarray(voxel_size, dtype=np.float64) * float(scale))[group[rows]][:, None]     # size[g] * scale, rounded once
    p = f[rows, :3]
    if variant == "recip":
        q = p * (1.0 / vs)
    elif variant == "fp32":
        with np.errstate(over="ignore", under="ignore"):
            q = (p.astype(np.float32) / vs.astype(np.float32)).astype(np.float64)
    else:
        q = p / vs
    q = np.floor(q) if variant == "floor" else np.trunc(q)
    if not np.all((q >= -KEY_LIMIT) & (q < KEY_LIMIT)):
        raise Refused("ERR_CAPACITY", "voxel index beyond +-2^19")
    v = q.astype(np.int64) + KEY_LIMIT
    key = (group[rows] << 60) | (v[:, 0] << 40) | (v[:, 1] << 20) | v[:, 2]       # one word per (group, voxel)
    if variant == "last_wins":
        _, first = np.unique(key[::-1], return_index=True)
        first = len(key) - 1 - first
    else:
        _, first = np.unique(key, return_index=True)                              # first occurrence of each
    kept = rows[first]
    kept = kept[np.lexsort((kept, group[kept]))]                                  # group-major, then input index
    return (f[kept].copy(), kept) if return_index else f[kept].copy()


def chain(frame, max_range, min_range, label_max_range, voxel_labels, voxel_size, variant=None, ds=None, levels=False):
    """Preprocess, then VoxelDownsample at 0.5 (frame_downsample) and at 1.5 (source): pipeline/sageICP.cpp:57-67, 97-101.
    ds: another one-level down-sampling (the oracle's, for the reference's emission order).  levels: both clouds."""
    assert variant is None or variant in VARIANTS, variant
    cv = variant if variant in CROP_VARIANTS else None
    dv = variant if variant in VDS_VARIANTS else None
    cropped, idx = preprocess(frame, max_range, min_range, label_max_range, variant=cv, return_index=True)
    if ds is not None:
        assert variant is None
        fd = ds(cropped, voxel_labels, voxel_size, 0.5)
        src = ds(fd, voxel_labels, voxel_size, 1.5)
    else:
        stale = _rows(frame)[idx, 3] if variant == "stale_label" else None
        fd = voxel_downsample(cropped, voxel_labels, voxel_size, 0.5, variant=dv, _lookup_labels=stale)
        src = voxel_downsample(fd, voxel_labels, voxel_size, 1.5, variant=dv)
    return (fd, src) if levels else src


# ---- the literal per-point loops ----------------------------------------------------------------------------------------
def py_preprocess(frame, max_range, min_range, label_max_range):
    out = []
    for p in np.asarray(frame, dtype=np.float64).reshape(-1, 4).tolist():      # Python floats: 1e200 squared is inf, silently
        xx, yy, zz = p[0] * p[0], p[1] * p[1], p[2] * p[2]
        # point.head<3>().norm(): packet reduction under order 2
        norm = float(np.sqrt((xx + yy) + zz if SQNORM3_ORDER == 2 else xx + (yy + zz)))
        if norm < max_range and norm > min_range:
            out.append([p[0], p[1], p[2], 0.0 if norm > label_max_range else p[3]])
    return np.array(out).reshape(-1, 4)


def py_voxel_downsample(frame, voxel_labels, voxel_size, scale):
    """core/Preprocessing.cpp:44-84 restated: first point per voxel per group; emitted group by
    group in input order"""
    grids = [dict() for _ in voxel_labels]
    for p in frame:
        label = int(p[3])
        group = next((g for g, ls in enumerate(voxel_labels) if label in ls), -1)
        if group < 0:
            continue
        vs = voxel_size[group] * scale
        key = (int(p[0] / vs), int(p[1] / vs), int(p[2] / vs))
        if key not in grids[group]:
            grids[group][key] = p
    out = [p for g in grids for p in g.values()]
    return np.array(out).reshape(-1, 4)
