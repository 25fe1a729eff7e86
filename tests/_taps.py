"""Spike taps (include/snn_hip.h: snn_planes_view): the three plane layouts restated in numpy as index arithmetic, and what the three taps
must return for a plane set - the expected values of tests/test_gpu_taps.py.  tests/test_taps_cpu.py pins the restatement against the
layout helpers of tests/_planes.py on synthetic buffers."""
import numpy as np

ROWS, SPLIT4, WORD_MAJOR = 0, 1, 2
LAYOUTS = (ROWS, SPLIT4, WORD_MAJOR)


def word_index(layout: int, rows: int, words: int) -> np.ndarray:
    """int64 [rows, words]: where word w of row r lies inside one step's plane, as the header states it"""
    r, w = np.arange(rows, dtype=np.int64)[:, None], np.arange(words, dtype=np.int64)[None, :]
    if layout == ROWS:
        return r * words + w
    if layout == SPLIT4:
        assert words % 4 == 0
        return ((w // 4) * rows + r) * 4 + w % 4
    if layout == WORD_MAJOR:
        return w * rows + r
    raise ValueError(layout)


def rows_from_layout(raw_words: np.ndarray, T: int, rows: int, words: int, layout: int, step_stride: int = None) -> np.ndarray:
    """uint32 [T, rows, words] from the flat words behind a view's offset"""
    stride = rows * words if step_stride is None else int(step_stride)
    idx = word_index(layout, rows, words)
    flat = np.asarray(raw_words).reshape(-1)
    return np.stack([flat[t * stride + idx] for t in range(T)])


def view_fields(v) -> dict:
    return dict(offset=int(v.offset_bytes), stride=int(v.step_stride_words), rows=int(v.rows), words=int(v.words), layout=int(v.layout),
                steps_formed=int(v.steps_formed))


def read_view(ws, v, T: int) -> np.ndarray:
    """the planes a view names inside a workspace tensor (uint8, any device) as uint32 [T, rows, words]"""
    f = view_fields(v)
    raw = ws[f["offset"]: f["offset"] + T * f["stride"] * 4].cpu().numpy().view(np.uint32)
    return rows_from_layout(raw, T, f["rows"], f["words"], f["layout"], f["stride"])


def dense(rows_u32: np.ndarray, n_cols: int) -> np.ndarray:
    """uint32 [T, rows, words] -> bool [T, rows, n_cols] (padding bits dropped)"""
    a = np.ascontiguousarray(rows_u32.astype(np.uint32))
    T, R, W = a.shape
    return np.unpackbits(a.view(np.uint8).reshape(T, R, W * 4), axis=2, bitorder="little")[:, :, :n_cols].astype(bool)


def expected_counts(spk: np.ndarray, rows_per_group):
    """bool [T, rows, n_cols] -> (per_step int64 [T, groups], per_col int64 [groups, n_cols], per_row int64 [rows])"""
    T, R, Cc = spk.shape
    starts = np.concatenate([[0], np.cumsum(rows_per_group)]).astype(np.int64)
    per_step = np.zeros((T, len(rows_per_group)), dtype=np.int64)
    per_col = np.zeros((len(rows_per_group), Cc), dtype=np.int64)
    per_row = np.zeros(R, dtype=np.int64)
    for g in range(len(rows_per_group)):
        s = spk[:, starts[g]:starts[g + 1]]
        per_step[:, g] = s.sum(axis=(1, 2))
        per_col[g] = s.sum(axis=(0, 1))
        per_row[starts[g]:starts[g + 1]] = s.sum(axis=(0, 2))
    return per_step, per_col, per_row
