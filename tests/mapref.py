"""Plain Python restatement of VoxelHashMap::Update with the product's block pool, for the tests only.

The policy is written from the reference's text (core/VoxelHashMap.hpp:45-70 AddPoint, VoxelHashMap.cpp:149-184
Update / AddPoints / RemovePointsFarFromLocation), the pool from DESIGN.md's stated rules:

  * voxels are blocks with indices; a new voxel takes the top of the free stack, else the next fresh index;
  * remove_far tests each live block's FIRST point in ascending block order and pushes the evicted blocks on the
    free stack in that order (every far voxel goes: the product's default sweep, not the reference's
    erase-while-iterating);
  * pointcloud() lists the live blocks in ascending index, each block's points in their stored order.

Regions, slots and the hash table are not modelled: none of them is observable.  Everything is Python floats and
ints evaluated one operation at a time, so each sum below rounds exactly where the C++ expression does
(-ffp-contract=off on both sides of the product).

tests/pyref.py's PyMap keeps its voxels in dict order, which stops matching Pointcloud() after the first eviction;
this one is what the map-update tests compare bytes against."""
import os

import numpy as np

# the association of the eviction test's 3-term squared norm (csrc/sageicp_types.h, SAGE_SQNORM3_FAR): the library
# and the oracle follow this variable, and so does this restatement
SQNORM3_ORDER = 0 if os.environ.get("SAGE_SQNORM3_ORDER", "2") == "0" else 2

KEY_LIMIT = 1 << 20         # |voxel index| < 2^20, else the whole update is refused with the map unchanged


def quat_to_mat(q):
    """se3_math.h quat_to_mat, operation for operation"""
    x, y, z, w = (float(v) for v in q[:4])
    xx, yy, zz = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    return (1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy),
            2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx),
            2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy))


def transform(pose, pts):
    """R0*x + R1*y + R2*z + t, left to right (se3_math.h mat_apply, k_up_keys); the label is carried over"""
    R = quat_to_mat(pose)
    t = [float(v) for v in pose[4:7]]
    out = []
    for x, y, z, l in np.asarray(pts, dtype=np.float64).reshape(-1, 4).tolist():
        out.append((R[0] * x + R[1] * y + R[2] * z + t[0],
                    R[3] * x + R[4] * y + R[5] * z + t[1],
                    R[6] * x + R[7] * y + R[8] * z + t[2], l))
    return out


class RefusedUpdate(ValueError):
    pass


class MapRef:
    def __init__(self, voxel_size, max_distance, basic=20, critical=20, basic_labels=(40, 44, 48, 49, 50, 70, 72)):
        self.vs, self.md = float(voxel_size), float(max_distance)
        self.basic, self.critical = int(basic), int(critical)
        self.basic_labels = tuple(int(l) for l in basic_labels)
        self.blocks = []        # per block index: list of (x, y, z, l), or None while the block is free
        self.keys = []          # per block index: its voxel
        self.index = {}         # voxel -> block index
        self.free = []          # stack of free block indices

    # ---- VoxelHashMap.cpp:162-174 + VoxelHashMap.hpp:45-70 ----
    def _voxel(self, p):
        return (int(p[0] / self.vs), int(p[1] / self.vs), int(p[2] / self.vs))     # int(): truncation toward zero

    def add_points(self, pts):
        pts = [tuple(float(v) for v in p) for p in (pts.tolist() if isinstance(pts, np.ndarray) else pts)]
        for p in pts:           # a dry pass first: a refused call changes nothing
            if not all(abs(p[a] / self.vs) < KEY_LIMIT for a in range(3)):
                raise RefusedUpdate("voxel index beyond +-2^20")
        for p in pts:
            key = self._voxel(p)
            b = self.index.get(key)
            if b is None:
                if self.free:
                    b = self.free.pop()
                    self.blocks[b], self.keys[b] = [p], key
                else:
                    b = len(self.blocks)
                    self.blocks.append([p])
                    self.keys.append(key)
                self.index[key] = b
                continue
            blk = self.blocks[b]
            if len(blk) < self.basic:
                blk.append(p)
                continue
            label = int(p[3])
            if label == 0:
                continue
            if label in self.basic_labels:
                self._replace_first_unlabelled(blk, p)
            elif len(blk) < self.basic + self.critical:
                blk.append(p)
            else:
                self._replace_first_unlabelled(blk, p)

    @staticmethod
    def _replace_first_unlabelled(blk, p):
        for j, e in enumerate(blk):
            if int(e[3]) == 0:
                blk[j] = p
                break

    # ---- VoxelHashMap.cpp:176-184 over the block pool ----
    def remove_far(self, origin):
        ox, oy, oz = (float(v) for v in origin)
        max2 = self.md * self.md
        for b, blk in enumerate(self.blocks):
            if blk is None:
                continue
            dx, dy, dz = blk[0][0] - ox, blk[0][1] - oy, blk[0][2] - oz
            xx, yy, zz = dx * dx, dy * dy, dz * dz
            d2 = xx + (yy + zz) if SQNORM3_ORDER == 0 else (xx + yy) + zz
            if d2 > max2:
                del self.index[self.keys[b]]
                self.blocks[b] = None
                self.free.append(b)

    # ---- VoxelHashMap.cpp:149-160 ----
    def update(self, pts, pose):
        self.add_points(transform(pose, pts))
        self.remove_far(pose[4:7])

    def pointcloud(self):
        rows = [p for blk in self.blocks if blk is not None for p in blk]
        return np.array(rows, dtype=np.float64).reshape(-1, 4)

    def size(self):
        return sum(len(blk) for blk in self.blocks if blk is not None)

    def num_voxels(self):
        return len(self.index)

    def count(self, key):
        b = self.index.get(tuple(key))
        return 0 if b is None else len(self.blocks[b])
