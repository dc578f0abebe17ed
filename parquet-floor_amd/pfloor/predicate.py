"""Row predicates of a filtered read. A list of them is a conjunction (AND).

    Range(column, lo=None, hi=None)   present and lo <= v <= hi (None: unbounded)
    Eq(column, v)                     Range(column, v, v)
    IsNull(column) / NotNull(column)

`column` is a column's index in the file or its name (a leaf's dotted path, or the first path element where that
names one leaf). Values become the PLAIN bytes of the column's physical type, which is what the GPU filter
(pf_decode_row_group_filter), the page index (ParquetFile.candidate_rows) and the Bloom filters compare: INT32 / INT64
as signed integers, FLOAT / DOUBLE by IEEE order, BYTE_ARRAY unsigned bytewise with a proper prefix first. Unsigned
and decimal logical orders are not covered."""
import struct

from ._native import PRED_IS_NULL, PRED_NOT_NULL, PRED_RANGE

BOOLEAN, INT32, INT64, INT96, FLOAT, DOUBLE, BYTE_ARRAY, FIXED_LEN_BYTE_ARRAY = range(8)


def plain_bytes(value, physical_type):
    """The PLAIN encoding of one value of the physical type (BYTE_ARRAY: without the length prefix). An int that does
    not fit the type, or a value of the wrong kind, is a ValueError."""
    t = physical_type
    if t == BOOLEAN:
        if isinstance(value, bool) or (isinstance(value, int) and value in (0, 1)):
            return bytes([int(value)])
        raise ValueError(f"BOOLEAN takes True / False (or 0 / 1), not {value!r}")
    if t in (INT32, INT64):
        if isinstance(value, bool) or not isinstance(value, int):
            raise ValueError(f"{'INT32' if t == INT32 else 'INT64'} takes an int, not {value!r}")
        bits = 32 if t == INT32 else 64
        if not -(1 << (bits - 1)) <= value < (1 << (bits - 1)):
            raise ValueError(f"{value} does not fit a signed {bits}-bit column")
        return int(value).to_bytes(bits // 8, "little", signed=True)
    if t in (FLOAT, DOUBLE):
        if isinstance(value, bool) or not isinstance(value, (int, float)):
            raise ValueError(f"{'FLOAT' if t == FLOAT else 'DOUBLE'} takes a float, not {value!r}")
        try:
            return struct.pack("<f" if t == FLOAT else "<d", float(value))
        except OverflowError as e:
            raise ValueError(f"{value} does not fit a FLOAT column") from e
    if t == BYTE_ARRAY:
        if isinstance(value, str):
            return value.encode("utf-8")
        if isinstance(value, (bytes, bytearray, memoryview)):
            return bytes(value)
        raise ValueError(f"BYTE_ARRAY takes bytes or str, not {value!r}")
    raise ValueError(f"no range predicate over physical type {t}")


class Predicate:
    op = None

    def __init__(self, column):
        self.column = column

    def bounds(self, physical_type):
        """(lo, hi): the bounds' PLAIN bytes, None where unbounded."""
        return None, None

    def __repr__(self):
        return f"{type(self).__name__}({self.column!r})"


class Range(Predicate):
    op = PRED_RANGE

    def __init__(self, column, lo=None, hi=None):
        super().__init__(column)
        self.lo, self.hi = lo, hi

    def bounds(self, physical_type):
        return (None if self.lo is None else plain_bytes(self.lo, physical_type),
                None if self.hi is None else plain_bytes(self.hi, physical_type))

    def __repr__(self):
        return f"{type(self).__name__}({self.column!r}, {self.lo!r}, {self.hi!r})"


class Eq(Range):
    def __init__(self, column, v):
        if v is None:
            raise ValueError("Eq(column, None): use IsNull(column)")
        super().__init__(column, v, v)

    def __repr__(self):
        return f"Eq({self.column!r}, {self.lo!r})"


class IsNull(Predicate):
    op = PRED_IS_NULL


class NotNull(Predicate):
    op = PRED_NOT_NULL


def resolve(columns, column):
    """The index of `column` (an index, a dotted path or a top-level name) among a file's ColumnDescriptors."""
    if isinstance(column, int) and not isinstance(column, bool):
        if not 0 <= column < len(columns):
            raise ValueError(f"no column {column}")
        return column
    hits = [c.index for c in columns if ".".join(c.path) == column] or [c.index for c in columns if c.path[0] == column]
    if len(hits) != 1:
        raise ValueError(f"column {column!r} names {len(hits)} leaves")
    return hits[0]


def bind(preds, columns, chunk_of):
    """Predicates -> the (chunk, op, lo, hi) tuples GpuDecoder.decode(predicates=...) takes. columns: the file's
    ColumnDescriptors; chunk_of: {column index: its position in the batch}."""
    out = []
    for p in preds:
        col = resolve(columns, p.column)
        lo, hi = p.bounds(columns[col].physical_type)
        out.append((chunk_of[col], p.op, lo, hi))
    return out
