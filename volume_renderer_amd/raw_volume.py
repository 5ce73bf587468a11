"""Python mirror of ``mex/matlab/RawVolume.m``: a ``Volume`` whose voxels stay in their native
element type until they are on the GPU.

``Volume`` casts every dataset to single, so it crosses the host link at four bytes per voxel.  A
``RawVolume`` keeps the uint8 / uint16 / int16 (here also float16) array in ``RawData``; the binding
sends it in its own width and the upload's pad pass widens it to single on the device.  The resident
volume and every image are bit for bit those of ``Volume(RawData.astype(np.float32))`` -- or, with
``Unorm`` (uint8 / uint16 only), of ``Volume(RawData.astype(np.float32) / np.float32(255))``
(``65535`` for uint16).  The illumination LUT and the gradient volumes stay single ``Volume``s.

``Data`` (inherited) holds a 1x1 single placeholder and is not read while ``RawData`` is set.
Assigning ``RawData`` or ``Unorm`` stamps ``TimeLastUpdate``; after an in-place edit call ``touch()``.
"""
from __future__ import annotations

import numpy as np

from .mex import dtype_code, timestamp
from .volume import Volume


class RawVolume(Volume):
    """Volume with a native-typed ``RawData`` and a logical ``Unorm`` (RawVolume.m)."""

    def __init__(self, data, unorm: bool = False):
        super().__init__(np.float32(0))
        self._raw = None
        self._unorm = bool(unorm)
        self.RawData = data

    @property
    def RawData(self):
        return self._raw

    @RawData.setter
    def RawData(self, data) -> None:
        a = np.asarray(data)
        if a.size:
            if a.dtype == np.float32:
                raise TypeError("RawData must be uint8, uint16, int16 or float16 (use Volume for single data)")
            dtype_code(a.dtype)  # TypeError for a type volumes cannot have
            if a.ndim > 3:
                raise ValueError("RawData must have at most 3 dimensions")
            if self._unorm and a.dtype not in (np.uint8, np.uint16):
                raise TypeError("Unorm is for uint8 / uint16 data only")
        self._raw = np.asfortranarray(a) if a.size else None
        self.TimeLastUpdate = timestamp()

    @property
    def Unorm(self) -> bool:
        return self._unorm

    @Unorm.setter
    def Unorm(self, value) -> None:
        value = bool(value)
        if value and self._raw is not None and self._raw.dtype not in (np.uint8, np.uint16):
            raise TypeError("Unorm is for uint8 / uint16 data only")
        self._unorm = value
        self.TimeLastUpdate = timestamp()

    def size(self):
        return self._raw.shape if self._raw is not None else super().size()

    def min(self):
        """The smallest voxel value as rendered (VolumeRender's absorption check reads it)."""
        if self._raw is None:
            return super().min()
        m = np.float32(self._raw.min())
        return m / np.float32(np.iinfo(self._raw.dtype).max) if self._unorm else m
