"""The two layouts of the downlink model delta, and their descriptor tables for ``ams_student_apply_delta``.

The payload that ``SemanticNetwork.delta_payload`` writes (reference run.py:316-336) has no header: the strategy, which both ends know from
their configuration, decides which variables it covers.

* trainable layout (every ``coord_desc_*`` strategy): ``spec.trainable`` in arena order, the order of ``curr_mask`` / ``train_params``;
* all-variables layout (``full_model``): ``spec.all_variable_names()``, the GraphDef order of every model variable (trainables and BN
  statistics interleaved), the key order of ``engine.get_variables()``.

Bytes: per variable ``np.packbits(mask.flatten())`` (big-endian bits, each variable starting on a byte), then the masked values of every
variable in the same order as little-endian fp16.  In the q8 format (``FORMATS``) the mask section is followed by one little-endian f32 scale
per variable of the layout and one int8 code of (value - base) per masked element instead.  This module is the one place that knows the two
orders; it holds no numerics.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Tuple

from . import hip
from .spec import StudentSpec

TRAINABLE, ALL_VARIABLES = "trainable", "all_variables"
# what follows the mask section: fp16 = the masked values as fp16 (the reference's payload); q8 = one f32 scale per variable of the layout,
# then one int8 code of (value - base) per masked element (include/ams_hip.h: ams_student_encode_delta_q8)
FP16, Q8 = "fp16", "q8"
FORMATS = (FP16, Q8)


def check_format(fmt: str) -> str:
    if fmt not in FORMATS:
        raise ValueError("delta format %r: one of %s" % (fmt, ", ".join(FORMATS)))
    return fmt


def layout_kind(train_strategy: str) -> str:
    if train_strategy == "full_model":
        return ALL_VARIABLES
    if "coord_desc_" in train_strategy:
        return TRAINABLE
    raise ValueError("no delta layout for train_strategy %r" % (train_strategy,))


@dataclass(frozen=True)
class DeltaEntry:
    name: str
    region: int           # hip.REGION_PARAMS or hip.REGION_STATS
    offset: int           # first element inside the region
    count: int
    mask_offset: int      # byte offset of the variable's mask bits in the payload


@dataclass(frozen=True)
class DeltaLayout:
    kind: str
    entries: Tuple[DeltaEntry, ...]
    mask_bytes: int
    n_elements: int
    _table: list = field(default_factory=list, repr=False, compare=False)

    @property
    def max_payload_bytes(self) -> int:
        """every element masked: the mask section plus two bytes per element"""
        return self.mask_bytes + 2 * self.n_elements

    @property
    def max_payload_bytes_q8(self) -> int:
        """the q8 format, every element masked: the mask section, one f32 scale per variable, one byte per element"""
        return self.mask_bytes + 4 * len(self.entries) + self.n_elements

    def payload_limit(self, fmt: str) -> int:
        return self.max_payload_bytes_q8 if check_format(fmt) == Q8 else self.max_payload_bytes

    def table(self):
        """the entries as a C array of ams_delta_var (built once)"""
        if not self._table:
            arr = (hip.DeltaVar * len(self.entries))()
            for d, e in zip(arr, self.entries):
                d.region, d.reserved, d.offset, d.count, d.mask_offset = e.region, 0, e.offset, e.count, e.mask_offset
            self._table.append(arr)
        return self._table[0]


def delta_layout(spec: StudentSpec, train_strategy: str) -> DeltaLayout:
    """The ordered descriptors of the payload a server running ``train_strategy`` sends, with its mask section and largest size."""
    kind = layout_kind(train_strategy)
    names = [v.name for v in spec.trainable] if kind == TRAINABLE else spec.all_variable_names()
    entries, mask, n = [], 0, 0
    for name in names:
        v = spec.by_name[name]
        entries.append(DeltaEntry(name, hip.REGION_PARAMS if v.trainable else hip.REGION_STATS, v.offset, v.size, mask))
        mask += (v.size + 7) // 8
        n += v.size
    return DeltaLayout(kind, tuple(entries), mask, n)
