"""Exactly decodable grids for the post-processing kernels (csrc/snn_post.h): inputs on which every decoded box is exact in fp32
and every pair of scores that is ever compared is either equal by construction or well apart (test infrastructure, host only; the
builder next to tests/_exact_grid.py).

Exact decode: size deltas are 0 (exp(0) == 1 in every implementation), centre deltas are dyadic (RPN k/8 or finer; detector
1.25 k/8, which BoxCoder's /10 turns into exactly k/64), anchors and proposals are integers.  Boxes are then bit-equal between device
and oracle, every IoU is the same fp32 number on both sides, and the order of the output is decided by construction: nothing is
left for a tolerance but the VALUE of a score (device expf against torch's exp, tests/_util.SCORE_ATOL).

Separated scores: logits come from small dyadic grids.  "Equal by construction" = the same logit (RPN), the same logits row and the
same logit inside it (detector).  Every other pair of scores that can meet in a sort, a merge or a list is at least SCORE_GAP apart
in the oracle, and every score is at least SCORE_GAP away from the score threshold, except sigmoid(0) == 0.5 against
score_thresh == 0.5, which is exact on both sides.  SCORE_GAP = 1e-4 = 50 x SCORE_ATOL: a condition on the INPUTS (drawn by
rejection until it holds), not a measurement.

Every builder uses np.random.default_rng(seed) with a fixed seed, checks its own preconditions and raises if one fails, and reports how
many of its decisions are planted edges (``planted``): pairs whose IoU equals the NMS threshold and decide a box's fate, tie groups
that straddle a cut (top-k, post_nms_top_n, detections_per_img), ties between entries of different lists that end up side by side.

The local models below (greedy_nms, rpn_model, det_model) restate the selection AFTER the oracle's decode with switches for
deliberately wrong variants; tests/test_post_grid_cpu.py shows that they equal the oracle with the switches off and that every
switch changes the result on the specs that plant its edge."""
import functools
from fractions import Fraction
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from oracle import post_oracle as PO
from oracle import torchvision_restated as TV

SCORE_GAP = 1e-4
BOX_WEIGHTS = (10.0, 10.0, 5.0, 5.0)


def f32_floor(t: float) -> np.float32:
    """largest fp32 <= t (what the library is handed for an NMS threshold t)"""
    f = np.float32(t)
    return np.nextafter(f, np.float32(-np.inf)) if float(f) > t else f


# ---- the local greedy loop, with the wrong variants as switches -------------------------------------------------------------------------
def greedy_nms(boxes: np.ndarray, thr: float, ge: bool = False, float_thr: bool = False, max_keep: Optional[int] = None,
               stats: Optional[dict] = None) -> List[int]:
    """boxes fp32 [n, 4] of ONE category in visiting order -> kept indices.  IoU in fp32 with box_iou's operation order, compared as a
    double with the double threshold.  ge: `>=` in place of `>`; float_thr: the threshold rounded to the nearest fp32 first.
    stats['edges'] counts the comparisons of a kept box with a live one whose IoU equals fp32(thr): the decisions made on the edge."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    n = b.shape[0]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    t = float(np.float32(thr)) if float_thr else float(thr)
    edge = float(np.float32(thr))
    dead = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        if max_keep is not None and len(keep) >= max_keep:
            break
        keep.append(i)
        r = np.nonzero(~dead[i + 1:])[0] + i + 1
        if r.size == 0:
            continue
        w = np.maximum(np.float32(0), np.minimum(b[i, 2], b[r, 2]) - np.maximum(b[i, 0], b[r, 0]))
        h = np.maximum(np.float32(0), np.minimum(b[i, 3], b[r, 3]) - np.maximum(b[i, 1], b[r, 1]))
        inter = w * h
        with np.errstate(invalid="ignore", divide="ignore"):
            iou = (inter / ((area[i] + area[r]) - inter)).astype(np.float64)
        if stats is not None:
            stats["edges"] = stats.get("edges", 0) + int((iou == edge).sum())
        dead[r[(iou >= t) if ge else (iou > t)]] = True
    return keep


ROUNDS_UP = (0.3, 0.6, 0.8)               # thresholds whose nearest fp32 lies above the decimal
# Which wrong comparison a pair with IoU == fp32(t) tells from `float IoU > double t`:
#   t = 0.5 (an fp32 number)     `>=`                    (and `>=` against the float threshold)
#   t = 0.3, 0.6, 0.8            the float threshold     (fp32(t) > t: the pair is suppressed, `iou > fp32(t)` keeps it)
#   t = 0.7 (fp32(t) < t)        `>=` against the float threshold (the pair is kept; `iou >= fp32(t)` suppresses it)
NMS_VARIANTS = ((dict(ge=True), (0.5,)), (dict(float_thr=True), ROUNDS_UP), (dict(ge=True, float_thr=True), (0.5, 0.7)))


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def edge_is_visible(model, spec, expected) -> bool:
    """does the OUTPUT (after every cut) depend on a decision made on the IoU edge: the wrong comparison that the spec's threshold can
    tell apart changes the local model's result.  A condition on the inputs, evaluated on the host."""
    return all(not _same(model(spec, **kw)[0], expected) for kw, thrs in NMS_VARIANTS if spec["nms"] in thrs)


def _tie_straddles(sorted_scores: np.ndarray, cut: int) -> bool:
    """does position `cut` of a sorted list fall inside a group of equal scores"""
    return 0 < cut < len(sorted_scores) and sorted_scores[cut - 1] == sorted_scores[cut]


# ========================================================================================================================================
# NMS, called directly
# ========================================================================================================================================
NMS_THRESHOLDS = (0.3, 0.5, 0.6, 0.7, 0.8)
NMS_SIZES = (2, 63, 64, 65, 128, 129, 193)
# boxes of width w shifted by d along one axis: IoU = (w - d) / (w + d)
NMS_PAIR = {0.3: (130, 70), 0.5: (30, 10), 0.6: (40, 10), 0.7: (170, 30), 0.8: (90, 10)}
# (suppressor, victim) positions in score order.  Same word: every pair of the bits 0, 31, 32, 63; adjacent words: all 16 combinations
_SAME = [[(0, 31), (32, 63)], [(0, 63), (31, 32)], [(0, 32), (31, 63)]]
_ADJ = [[(0, 64), (31, 95), (32, 96), (63, 127)], [(0, 95), (31, 64), (32, 127), (63, 96)],
        [(0, 96), (31, 127), (32, 64), (63, 95)], [(0, 127), (31, 96), (32, 95), (63, 64)]]
NMS_LAYOUTS = len(_SAME) + len(_ADJ)


def _layout_pairs(layout: int, n: int) -> List[Tuple[int, int]]:
    if layout < len(_SAME):
        pairs = [(64 * w + a, 64 * w + b) for w in range(4) for a, b in _SAME[layout]]
    else:
        pairs = [(64 * w + a, 64 * w + b) for w in range(0, 4, 2) for a, b in _ADJ[layout - len(_SAME)]]
    pairs = [p for p in pairs if p[1] < n]
    used = {q for p in pairs for q in p}
    if n >= 2 and n - 1 not in used and n - 2 not in used:
        pairs.append((n - 2, n - 1))                                  # the last candidate is always a victim
    return pairs


@functools.lru_cache(maxsize=None)
def nms_case(n: int, thr: float, ncat: int, layout: int) -> dict:
    """n integer boxes, one per 256 x 256 cell (mutually disjoint) except the planted victims, which share the cell of their suppressor
    shifted along x or y: IoU exactly thr (every even pair), or the nearest integer ratio on either side (d -/+ 1).  With ncat > 1 some
    'above' pairs are split over two categories (no suppression).  Scores are distinct dyadics; the input order is shuffled."""
    rng = np.random.default_rng(7000 + 131 * n + 17 * layout + int(round(thr * 10)) + 1000 * ncat)
    w0, d0 = NMS_PAIR[thr]
    assert Fraction(w0 - d0, w0 + d0) == Fraction(int(round(thr * 10)), 10)
    cell = np.arange(n)
    boxes = np.zeros((n, 4), dtype=np.float64)
    cat = rng.integers(0, ncat, size=n)
    kinds = {}
    for p in range(n):
        cx, cy = 256 * (p % 16) + 8, 256 * (p // 16) + 8
        bw, bh = int(rng.integers(4, 200)), int(rng.integers(4, 200))
        boxes[p] = (cx, cy, cx + bw, cy + bh)
    for j, (ps, pv) in enumerate(_layout_pairs(layout, n)):
        kind = "edge" if j % 2 == 0 or n == 2 else ("above" if (j // 2 + layout) % 2 == 0 else "below")
        d = d0 + {"edge": 0, "above": -1, "below": 1}[kind]
        x, y = 256 * (ps % 16) + 8, 256 * (ps // 16) + 8
        other = int(rng.integers(20, 40))
        if (j + layout) % 2 == 0:                                     # shifted along x
            boxes[ps] = (x, y, x + w0, y + other)
            boxes[pv] = (x + d, y, x + d + w0, y + other)
        else:
            boxes[ps] = (x, y, x + other, y + w0)
            boxes[pv] = (x, y + d, x + other, y + d + w0)
        cat[pv] = cat[ps]
        if ncat > 1 and kind == "above" and j % 4 == 1:
            cat[pv] = (cat[ps] + 1) % ncat
            kind = "cross"
        kinds[(ps, pv)] = kind
    assert boxes.max() < 2 ** 13
    scores = (n - cell).astype(np.float64) / 256.0                    # position p in score order has score (n - p) / 256
    # what the planted pairs decide, from the local loop category by category
    st = {}
    for c in range(ncat):
        greedy_nms(boxes[cat == c].astype(np.float32), thr, stats=st)
    perm = rng.permutation(n)
    return dict(boxes=torch.from_numpy(boxes[perm].astype(np.float32)), scores=torch.from_numpy(scores[perm].astype(np.float32)),
                idxs=torch.from_numpy(cat[perm].astype(np.int64)), thr=thr, kinds=kinds,
                planted={"iou_edges": int(st.get("edges", 0))})


# ========================================================================================================================================
# RPN
# ========================================================================================================================================
# anchor size / stride whose neighbouring grid positions sit exactly on the threshold at zero deltas: (size - stride) / (size + stride);
# (H0, W0) = the largest level's grid, chosen so that some positions stay unclipped along each axis
RPN_GEOMETRY = {0.5: (24, 8, 8, 10), 0.3: (26, 14, 8, 10), 0.6: (32, 8, 8, 10), 0.7: (34, 6, 10, 12), 0.8: (72, 8, 12, 14)}
RPN_MIN_SIZE = 4.0
RPN_SPECS = {
    # name: nms, N, pre, post, score_thresh
    "r_t5_all": dict(nms=0.5, N=1, pre=1000, post=64, score_thresh=0.0),
    "r_t3_cut": dict(nms=0.3, N=3, pre=64, post=5, score_thresh=0.0),
    "r_t6_w65": dict(nms=0.6, N=1, pre=65, post=5, score_thresh=0.0),
    "r_t7_thr": dict(nms=0.7, N=3, pre=1000, post=5, score_thresh=0.5),
    "r_t8_w65": dict(nms=0.8, N=3, pre=65, post=1000, score_thresh=0.0),
    "r_t3_thr": dict(nms=0.3, N=1, pre=1000, post=1000, score_thresh=0.5),
    "r_t7_w64": dict(nms=0.7, N=1, pre=64, post=1000, score_thresh=0.0),
    "r_t8_all": dict(nms=0.8, N=3, pre=1000, post=64, score_thresh=0.0),
    "r_t6_cut": dict(nms=0.6, N=3, pre=64, post=5, score_thresh=0.5),
    "r_t5_w65": dict(nms=0.5, N=3, pre=65, post=5, score_thresh=0.0),
    # logits on the k/64 grid, distinct inside every level: top-k has nothing to choose
    "r_t7_dist": dict(nms=0.7, N=1, pre=1000, post=1000, score_thresh=0.0, distinct=True),
}
RPN_WRAPPED = "r_t3_cut"                   # also goes through RegionProposalNetwork with a stored head


def rpn_geometry(nms: float) -> dict:
    size, stride, H0, W0 = RPN_GEOMETRY[nms]
    assert Fraction(size - stride, size + stride) == Fraction(int(round(nms * 10)), 10)
    canvas = (H0 * stride, W0 * stride)
    grids = [(H0, W0), (H0 // 2, W0 // 2), (1, 1)]
    sizes = ((size, 2 * size), (2 * size, 4 * size), (4 * size, 8 * size))
    return dict(canvas=canvas, grids=grids, sizes=sizes, ratios=((1.0,),) * 3, A=2, stride=stride, size=size)


def _rpn_decode_all(obj, dl, geo, N, dtype):
    """every anchor of every image decoded as the oracle does (rpn.py:636-664), in `dtype`"""
    feats = [torch.empty((N, 1) + tuple(g)) for g in geo["grids"]]
    images = TV.ImageList(torch.empty((N, 3) + tuple(geo["canvas"])), [geo["canvas"]] * N)
    anchors = TV.AnchorGenerator(geo["sizes"], geo["ratios"])(images, feats)
    deltas = torch.cat([PO._flatten_level(d, 4) for d in dl], dim=1).reshape(-1, 4)
    return TV.BoxCoder((1.0, 1.0, 1.0, 1.0)).decode(deltas.to(dtype), [a.to(dtype) for a in anchors]).view(N, -1, 4)


def _min_size_plan(geo, w_img):
    """(x, delta) per width: level-0 columns and dyadic x deltas of anchor 0 whose clipped boxes are exactly RPN_MIN_SIZE and
    RPN_MIN_SIZE - 0.5 wide in an image w_img wide, or None"""
    size, stride = geo["size"], geo["stride"]
    plan = []
    for width in (RPN_MIN_SIZE, RPN_MIN_SIZE - 0.5):
        found = None
        for x in range(geo["grids"][0][1] - 1, -1, -1):
            for k in sorted(range(-256, 257), key=abs):
                x1 = x * stride - size / 2 + (k / 64.0) * size        # exact in fp64: small dyadics
                if 0 <= x1 and w_img - x1 == width and x1 + size > w_img:
                    found = (x, k / 64.0)
                    break
            if found:
                break
        if found is None:
            return None
        plan.append(found)
    return plan


def rpn_image_sizes(geo, N):
    """image sizes a few pixels inside the canvas (boxes get clipped), each with a width that admits the two min_size edges"""
    Hc, Wc = geo["canvas"]
    out, w = [], Wc
    for i in range(N):
        w -= 1
        while _min_size_plan(geo, w) is None:
            w -= 1
        out.append((Hc - (3, 0, 7)[i], w))
    assert w > Wc // 2
    return out


def _plant_min_size(geo, image_sizes, dl, obj, tops=(4.0, 4.0)):
    """per image two anchors of level 0 (anchor 0) whose clipped boxes are exactly RPN_MIN_SIZE and RPN_MIN_SIZE - 0.5 wide: a dyadic
    x delta pushes them against the right image border; top logit, so that they are candidates.  Returns the planted (image, y, x, width)"""
    size, stride = geo["size"], geo["stride"]
    H0, W0 = geo["grids"][0]
    out = []
    for i, (_, w_img) in enumerate(image_sizes):
        rows = iter(range(1, H0 - 1))
        for width, found, top in zip((RPN_MIN_SIZE, RPN_MIN_SIZE - 0.5), _min_size_plan(geo, w_img), tops):
            y = next(rows)
            dl[0][i, :, y, found[0]] = 0.0
            dl[0][i, 0, y, found[0]] = found[1]
            obj[0][i, 0, y, found[0]] = top
            out.append((i, y, found[0], width))
    return out


def rpn_model(spec: dict, ge: bool = False, float_thr: bool = False, tie_reversed: bool = False, cut_later: int = 0,
              stats: Optional[dict] = None):
    """the selection after the oracle's candidates (clip, filters, NMS per level, merge, cut) restated on numpy with the wrong variants
    as switches -> (boxes, scores) per image.  tie_reversed: equal scores of different levels in DESCENDING level order;
    cut_later: post_nms_top_n + cut_later rows."""
    sp, geo = spec, spec["geo"]
    ks = [min(sp["pre"], h * w * geo["A"]) for h, w in geo["grids"]]
    level = np.concatenate([np.full(k, l) for l, k in enumerate(ks)])
    out_b, out_s = [], []
    for i, pre in enumerate(spec["expected"][2]):
        boxes = TV.clip_boxes_to_image(pre["proposals"], sp["image_sizes"][i]).numpy()
        prob = pre["objectness"].numpy()
        ok = ((boxes[:, 2] - boxes[:, 0]) >= np.float32(sp["min_size"])) & ((boxes[:, 3] - boxes[:, 1]) >= np.float32(sp["min_size"]))
        ok &= prob >= np.float32(sp["score_thresh"])
        rows = []                                                     # (score, level, rank inside the level, candidate)
        for l in range(len(ks)):
            cand = np.nonzero(ok & (level == l))[0]                  # already in score order (stable top-k)
            for r, c in enumerate(greedy_nms(boxes[cand], sp["nms"], ge=ge, float_thr=float_thr, stats=stats)):
                rows.append((float(prob[cand[c]]), l, r, int(cand[c])))
        rows.sort(key=lambda t: (-t[0], -t[1] if tie_reversed else t[1], t[2]))
        if stats is not None:
            sc = np.array([t[0] for t in rows])
            stats["cut_straddles"] = stats.get("cut_straddles", 0) + int(_tie_straddles(sc, sp["post"]))
            kept = rows[:sp["post"]]
            stats["cross_list_ties"] = stats.get("cross_list_ties", 0) + sum(
                1 for a, b in zip(kept[:-1], kept[1:]) if a[0] == b[0] and a[1] != b[1])
        rows = rows[:sp["post"] + cut_later]
        idx = np.array([t[3] for t in rows], dtype=np.int64)
        out_b.append(torch.from_numpy(boxes[idx].reshape(-1, 4)))
        out_s.append(torch.from_numpy(prob[idx]))
    return out_b, out_s


@functools.lru_cache(maxsize=None)
def rpn_spec(name: str) -> dict:
    """inputs, the oracle's expectation (stable top-k) and the planted counts of RPN_SPECS[name]; the logits are redrawn (same generator)
    until every cut the spec has falls inside a tie group"""
    sp = dict(RPN_SPECS[name])
    geo = rpn_geometry(sp["nms"])
    Hc, Wc = geo["canvas"]
    N, A = sp["N"], geo["A"]
    sp["image_sizes"] = rpn_image_sizes(geo, N)
    sp["min_size"] = RPN_MIN_SIZE
    rng = np.random.default_rng(9100 + sorted(RPN_SPECS).index(name))
    for attempt in range(200):
        obj, dl = [], []
        for (h, w) in geo["grids"]:
            if sp.get("distinct"):
                q = np.stack([rng.choice(np.arange(-256, 255), size=A * h * w, replace=False) for _ in range(N)]).reshape(N, A, h, w)
                obj.append(torch.from_numpy(q.astype(np.float32) / 64.0))
            else:
                obj.append(torch.from_numpy(rng.integers(-16, 17, size=(N, A, h, w)).astype(np.float32) / 4.0))
            d = np.zeros((N, A, 4, h, w), dtype=np.float32)
            moved = rng.random((N, A, 1, h, w)) < 0.2
            d[:, :, :2] = np.where(moved, rng.integers(-4, 5, size=(N, A, 2, h, w)) / 8.0, 0.0)     # centre deltas k/8, size deltas 0
            dl.append(torch.from_numpy(d.reshape(N, 4 * A, h, w)))
        small = _plant_min_size(geo, sp["image_sizes"], dl, obj, (4.0, 255.0 / 64.0) if sp.get("distinct") else (4.0, 4.0))
        args = (obj, dl, geo["canvas"], sp["image_sizes"], geo["sizes"], geo["ratios"], sp["pre"], sp["post"], sp["nms"],
                sp["score_thresh"], sp["min_size"])
        spec = dict(sp, name=name, geo=geo, obj=obj, dl=dl, small=small, oracle_args=args)
        spec["expected"] = PO.rpn_proposals(*args, stable_topk=True)
        st = {}
        rpn_model(spec, stats=st)
        topk_straddles = within_ties = 0
        for o in obj:
            flat = PO._flatten_level(o, 1).reshape(N, -1)
            srt = torch.sort(flat, dim=1, descending=True, stable=True)[0].numpy()
            k = min(sp["pre"], flat.shape[1])
            topk_straddles += sum(int(_tie_straddles(srt[i], k)) for i in range(N))
            within_ties += sum(int((np.diff(srt[i][:k]) == 0).sum()) for i in range(N))
        planted = {"iou_edges": st.get("edges", 0), "cut_straddles": st.get("cut_straddles", 0) + topk_straddles,
                   "topk_straddles": topk_straddles, "post_straddles": st.get("cut_straddles", 0),
                   "cross_list_ties": st.get("cross_list_ties", 0), "within_level_ties": within_ties}
        n0 = geo["grids"][0][0] * geo["grids"][0][1] * A
        want_topk = sp["pre"] < n0
        want_post = sp["post"] < 1000
        if not edge_is_visible(rpn_model, spec, spec["expected"][0]):
            continue
        if sp.get("distinct"):
            if planted["iou_edges"] >= 2 and within_ties == 0:
                break
        elif (planted["iou_edges"] >= 2 and planted["cross_list_ties"] >= 1 and (not want_topk or topk_straddles >= 1)
                and (not want_post or planted["post_straddles"] >= 1)):
            break
    else:
        raise AssertionError("%s: no draw plants every edge (last: %s)" % (name, planted))
    spec["planted"] = planted
    spec["attempts"] = attempt + 1
    _check_rpn_preconditions(spec)
    return spec


def _check_rpn_preconditions(spec):
    geo, N = spec["geo"], spec["N"]
    b32 = _rpn_decode_all(spec["obj"], spec["dl"], geo, N, torch.float32)
    b64 = _rpn_decode_all(spec["obj"], spec["dl"], geo, N, torch.float64)
    for i in range(N):
        c32 = TV.clip_boxes_to_image(b32[i], spec["image_sizes"][i])
        c64 = TV.clip_boxes_to_image(b64[i], spec["image_sizes"][i])
        if not (torch.equal(b32[i].double(), b64[i]) and torch.equal(c32.double(), c64)):
            raise AssertionError("%s: the fp32 decode is not exact" % spec["name"])
    # scores: the sigmoid of distinct grid logits is >= SCORE_GAP apart, and >= SCORE_GAP from the threshold unless the logit is 0
    grid = torch.arange(-256, 257, dtype=torch.float32) / 64.0 if spec.get("distinct") else torch.arange(-16, 17, dtype=torch.float32) / 4.0
    p = torch.sigmoid(grid).double().numpy()
    if not np.diff(p).min() >= SCORE_GAP:
        raise AssertionError("grid logits give scores closer than %g" % SCORE_GAP)
    off = np.abs(p - spec["score_thresh"])
    exact = (grid.numpy() == 0.0) & (spec["score_thresh"] == 0.5) & (p == 0.5)
    if not (off[~exact] >= SCORE_GAP).all():
        raise AssertionError("a grid score sits within %g of the score threshold" % SCORE_GAP)
    for o in spec["obj"]:
        if not np.isin(o.numpy(), grid.numpy()).all():
            raise AssertionError("a logit off the grid")
    widths = {w for (_, _, _, w) in spec["small"]}
    if widths != {RPN_MIN_SIZE, RPN_MIN_SIZE - 0.5}:
        raise AssertionError("min_size edges not planted")


def rpn_device_inputs(spec, device):
    """what ops.rpn_proposals takes: position-major logits [N*H*W, A] / deltas [N*H*W, 4A], grids, strides"""
    N = spec["N"]
    lg, de, hw, strides = [], [], [], []
    for o, d in zip(spec["obj"], spec["dl"]):
        H, W = o.shape[-2:]
        lg.append(o.permute(0, 2, 3, 1).reshape(N * H * W, -1).contiguous().to(device))
        de.append(d.permute(0, 2, 3, 1).reshape(N * H * W, -1).contiguous().to(device))
        hw.append((H, W))
        strides.append((spec["geo"]["canvas"][0] // H, spec["geo"]["canvas"][1] // W))
    return lg, de, hw, strides


# ========================================================================================================================================
# third radix pass: consecutive fp32 numbers
# ========================================================================================================================================
RADIX_CANVAS = (260, 510)
RADIX_GRIDS = [(130, 255), (32, 32), (32, 32)]           # 33 150 (> 32 768: two trips of the histogram's 1024-element loop), 1024, 1024
RADIX_SIZES = ((32,), (64,), (128,))


@functools.lru_cache(maxsize=None)
def radix_spec() -> dict:
    """A = 1, N = 2.  Level 0: 1024 consecutive fp32 numbers from +1.0 upwards at random positions among distinct lower fillers; level 1:
    the 1024 consecutive numbers from -1.0 downwards; level 2: those from +1.0 upwards.  All values of a level are distinct and the 1024
    of the cluster share the upper 22 bits of their keys, so only the third pass (10 bits) tells them apart."""
    rng = np.random.default_rng(9300)
    N = 2
    up = (np.uint32(0x3F800000) + np.arange(1024, dtype=np.uint32)).view(np.float32)
    down = (np.uint32(0xBF800000) + np.arange(1024, dtype=np.uint32)).view(np.float32)
    n0 = RADIX_GRIDS[0][0] * RADIX_GRIDS[0][1]
    fill = (-2.0 - np.arange(n0 - 1024) / 64.0).astype(np.float32)
    levels = []
    for vals in (np.concatenate([up, fill]), down, up):
        assert len(np.unique(vals)) == len(vals)
        levels.append(np.stack([vals[rng.permutation(len(vals))] for _ in range(N)]))
    for vals in (up, down):
        u = vals.view(np.uint32)
        key = np.where(u & 0x80000000, ~u, u | 0x80000000)
        assert len(np.unique(key >> 10)) == 1
    obj = [torch.from_numpy(v.reshape((N, 1) + g)) for v, g in zip(levels, RADIX_GRIDS)]
    return dict(N=N, obj=obj, canvas=RADIX_CANVAS, grids=RADIX_GRIDS, sizes=RADIX_SIZES, ratios=((1.0,),) * 3)


# ========================================================================================================================================
# detector
# ========================================================================================================================================
DET_SCORE_THRESH = 0.4
DET_SPECS = {
    "d_k5_big": dict(K=5, rois=[130, 64, 0], det=100, nms=0.5, fg=0.8),
    "d_k2_small": dict(K=2, rois=[65, 1], det=3, nms=0.3, fg=0.7),
    "d_k2_big": dict(K=2, rois=[130, 64, 0], det=3, nms=0.3, fg=0.8),
    "d_k5_small": dict(K=5, rois=[65, 1], det=3, nms=0.5, fg=0.7),
}
DET_IMAGE_SHAPES = [(1400, 1500), (1390, 1480), (700, 900)]


def _det_dictionary(K: int, rng) -> Tuple[np.ndarray, np.ndarray]:
    """about 12 rows of quarter-grid logits -> (rows [n, K] fp32, is_fg [n]).  Drawn by rejection until every two scores with different
    (row, logit) keys that can be compared (foreground scores above the threshold among themselves, background scores of rows without
    a foreground class among themselves) are SCORE_GAP apart and every foreground score is SCORE_GAP away from the threshold."""
    for _ in range(2000):
        rows = []
        for j in range(12):
            r = rng.integers(-12, 5, size=K).astype(np.float64) / 4.0
            kind = j % 3
            if kind == 0:                                             # one clear foreground class
                r[1 + int(rng.integers(K - 1))] = float(rng.integers(8, 17)) / 4.0
            elif kind == 1 and K > 2:                                 # two equal foreground logits: a cross-class tie
                a, b = rng.choice(np.arange(1, K), size=2, replace=False)
                r[a] = r[b] = float(rng.integers(8, 13)) / 4.0
            elif kind == 1:
                r[1] = float(rng.integers(4, 13)) / 4.0
            else:                                                     # no class above the threshold: the background path
                r[0] = float(rng.integers(4, 13)) / 4.0
            rows.append(r)
        rows = np.unique(np.array(rows, dtype=np.float32), axis=0)
        if len(rows) < 10:
            continue
        sc = torch.softmax(torch.from_numpy(rows), -1).double().numpy()
        fg_mask = sc[:, 1:] > DET_SCORE_THRESH
        is_fg = fg_mask.any(1)
        if np.abs(sc[:, 1:] - DET_SCORE_THRESH).min() < SCORE_GAP or is_fg.sum() < 6 or (~is_fg).sum() < 3:
            continue
        ok = True
        for pool in ([(sc[r, c], (r, rows[r, c])) for r in range(len(rows)) for c in range(1, K) if sc[r, c] > DET_SCORE_THRESH],
                     [(sc[r, 0], (r, rows[r, 0])) for r in range(len(rows)) if not is_fg[r]]):
            for a in range(len(pool)):
                for b in range(a + 1, len(pool)):
                    if pool[a][1] == pool[b][1]:
                        ok &= pool[a][0] == pool[b][0]                # equal by construction: bit-equal in the oracle
                    else:
                        ok &= abs(pool[a][0] - pool[b][0]) >= SCORE_GAP
        if ok and (K == 2 or any((r[1:] == r[1:].max()).sum() == 2 and f for r, f in zip(rows, is_fg))):
            return rows, is_fg
    raise AssertionError("no separated logits dictionary for K = %d" % K)


def det_model(spec: dict, ge: bool = False, float_thr: bool = False, tie_reversed: bool = False, cut_later: int = 0,
              stats: Optional[dict] = None):
    """the selection after the oracle's decode / softmax (all_scores, all_boxes) restated with the wrong variants as switches ->
    (boxes, scores, labels) per image, foreground rows then background rows.  tie_reversed: equal scores in DESCENDING candidate order
    (RoI * (K-1) + class - 1), in the class lists, the merge and the background list alike."""
    K, thr = spec["K"], np.float32(DET_SCORE_THRESH)
    sgn = -1 if tie_reversed else 1
    out = ([], [], [])
    for i in range(len(spec["rois"])):
        sc, bx = spec["expected"][3][i].numpy(), spec["expected"][4][i].numpy()
        R = sc.shape[0]
        big = ((bx[..., 2] - bx[..., 0]) >= np.float32(1e-2)) & ((bx[..., 3] - bx[..., 1]) >= np.float32(1e-2))
        fg = np.zeros((R, K), dtype=bool)
        fg[:, 1:] = sc[:, 1:] > thr
        rows = []
        for c in range(1, K):
            cand = sorted(np.nonzero(fg[:, c] & big[:, c])[0], key=lambda r: (-float(sc[r, c]), sgn * r))
            for r in greedy_nms(bx[cand, c], spec["nms"], ge=ge, float_thr=float_thr, stats=stats):
                rows.append((float(sc[cand[r], c]), int(cand[r]) * (K - 1) + c - 1, int(cand[r]), c))
        rows.sort(key=lambda t: (-t[0], sgn * t[1]))
        if stats is not None:
            s_ = np.array([t[0] for t in rows])
            stats["cut_straddles"] = stats.get("cut_straddles", 0) + int(_tie_straddles(s_, spec["det"]))
            kept = rows[:spec["det"]]
            stats["cross_list_ties"] = stats.get("cross_list_ties", 0) + sum(
                1 for a, b in zip(kept[:-1], kept[1:]) if a[0] == b[0] and a[3] != b[3])
            stats["same_class_ties"] = stats.get("same_class_ties", 0) + sum(
                1 for a, b in zip(kept[:-1], kept[1:]) if a[0] == b[0] and a[3] == b[3])
        rows = rows[:spec["det"] + cut_later]
        bgc = sorted(np.nonzero(~fg.any(1) & big[:, 0])[0], key=lambda r: (-float(sc[r, 0]), sgn * r))
        bgk = [bgc[r] for r in greedy_nms(bx[bgc, 0], spec["nms"], ge=ge, float_thr=float_thr, stats=stats)]
        if stats is not None:
            stats["bg_rows"] = stats.get("bg_rows", 0) + len(bgk)
            stats["bg_ties"] = stats.get("bg_ties", 0) + sum(1 for a, b in zip(bgk[:-1], bgk[1:]) if sc[a, 0] == sc[b, 0])
        b = [bx[t[2], t[3]] for t in rows] + [bx[r, 0] for r in bgk]
        out[0].append(torch.from_numpy(np.array(b, dtype=np.float32).reshape(-1, 4)))
        out[1].append(torch.from_numpy(np.array([t[0] for t in rows] + [sc[r, 0] for r in bgk], dtype=np.float32)))
        out[2].append(torch.from_numpy(np.array([t[3] for t in rows] + [0] * len(bgk), dtype=np.int64)))
    return out


@functools.lru_cache(maxsize=None)
def det_spec(name: str) -> dict:
    """inputs, the oracle's expectation and the planted counts of DET_SPECS[name].  Integer proposals on a coarse lattice (so that many
    are disjoint and more than detections_per_img survive), with duplicates, zero-area boxes, boxes reaching outside the image and
    planted pairs whose IoU is exactly the NMS threshold; centre deltas 1.25 k / 8, size deltas 0; logits rows from the dictionary."""
    sp = dict(DET_SPECS[name])
    K = sp["K"]
    rng = np.random.default_rng(9500 + sorted(DET_SPECS).index(name))
    w0, d0 = NMS_PAIR[sp["nms"]]
    shapes = DET_IMAGE_SHAPES[:len(sp["rois"])]
    for attempt in range(200):
        rows, is_fg = _det_dictionary(K, rng)
        fg_rows, bg_rows = np.nonzero(is_fg)[0], np.nonzero(~is_fg)[0]
        props, logits, reg = [], [], []
        for i, R in enumerate(sp["rois"]):
            H, W = shapes[i]
            p = np.zeros((R, 4))
            which = np.where(rng.random(R) < sp["fg"], rng.choice(fg_rows, size=R), rng.choice(bg_rows, size=R))
            d = np.zeros((R, K, 4))
            d[:, :, :2] = np.where(rng.random((R, K, 1)) < 0.4, 1.25 * rng.integers(-8, 9, size=(R, K, 2)) / 8.0, 0.0)
            for r in range(R):
                x, y = 100 * int(rng.integers(0, W // 100 + 1)), 100 * int(rng.integers(0, H // 100))
                p[r] = (x, y, x + int(rng.integers(30, 90)), y + int(rng.integers(30, 90)))
            for r in range(0, R - 1, 9):                              # planted: pairs on the threshold, duplicates, zero-area boxes
                kind = (r // 9) % 4
                if kind in (0, 1):
                    x, y = int(rng.integers(0, W - 2 * w0)), int(rng.integers(0, H - 2 * w0))
                    other = int(rng.integers(40, 80))
                    p[r] = (x, y, x + w0, y + other) if kind == 0 else (x, y, x + other, y + w0)
                    p[r + 1] = p[r] + ((d0, 0, d0, 0) if kind == 0 else (0, d0, 0, d0))
                    d[r] = d[r + 1] = 0.0
                    which[r] = which[r + 1] = rng.choice(fg_rows) if (r // 9) % 8 < 6 else rng.choice(bg_rows)
                elif kind == 2:
                    p[r + 1] = p[r]
                    d[r + 1] = d[r]
                else:
                    p[r + 1, 2] = p[r + 1, 0]
                    d[r + 1] = 0.0
            props.append(torch.from_numpy(p.astype(np.float32)))
            logits.append(torch.from_numpy(rows[which].reshape(R, K)))
            reg.append(torch.from_numpy(d.reshape(R, 4 * K).astype(np.float32)))
        spec = dict(sp, name=name, image_shapes=shapes, props=props, logits=torch.cat(logits), reg=torch.cat(reg), dictionary=rows)
        spec["expected"] = PO.det_postprocess(spec["logits"], spec["reg"], props, list(shapes), BOX_WEIGHTS, DET_SCORE_THRESH, sp["nms"],
                                              sp["det"])
        st = {}
        det_model(spec, stats=st)
        planted = {"iou_edges": st.get("edges", 0), "cut_straddles": st.get("cut_straddles", 0),
                   "cross_list_ties": st.get("cross_list_ties", 0), "same_class_ties": st.get("same_class_ties", 0),
                   "bg_rows": st.get("bg_rows", 0), "bg_ties": st.get("bg_ties", 0)}
        if not edge_is_visible(det_model, spec, spec["expected"][0]):
            continue
        if (planted["iou_edges"] >= 2 and planted["cut_straddles"] >= 1 and planted["same_class_ties"] >= 1 and planted["bg_ties"] >= 1
                and (K == 2 or planted["cross_list_ties"] >= 1)):
            break
    else:
        raise AssertionError("%s: no draw plants every edge (last: %s)" % (name, planted))
    spec["planted"] = planted
    spec["attempts"] = attempt + 1
    _check_det_preconditions(spec)
    return spec


def _check_det_preconditions(spec):
    coder = TV.BoxCoder(BOX_WEIGHTS)
    # the deltas are 1.25 k / 8 = 5 k / 32; fp32 (5 k / 32) / 10 is exactly k / 64, which the fp64 decode is handed as 10 k / 64
    d64 = spec["reg"].double().reshape(-1, spec["K"], 4).clone()
    k5 = d64[..., :2] * 32.0
    if not torch.equal(k5, torch.round(k5)) or bool((torch.remainder(k5, 5.0) != 0).any()) or bool((d64[..., 2:] != 0).any()):
        raise AssertionError("%s: deltas off the grid" % spec["name"])
    d64[..., :2] = (k5 / 5.0) * 10.0 / 64.0
    b64 = coder.decode(d64.reshape(-1, 4 * spec["K"]), [p.double() for p in spec["props"]])
    pos = 0
    for i, R in enumerate(spec["rois"]):
        c64 = TV.clip_boxes_to_image(b64[pos:pos + R], spec["image_shapes"][i])
        if not torch.equal(spec["expected"][4][i].double(), c64):
            raise AssertionError("%s: the fp32 decode is not exact (image %d)" % (spec["name"], i))
        pos += R
    for p in spec["props"]:
        if not torch.equal(p, torch.round(p)):
            raise AssertionError("proposals are not integers")


def det_padded_inputs(spec, device, fill_seed: int = 1):
    """the rows of the spec laid out [N, cap] with cap = the largest image, padding rows filled with other (finite) values"""
    K, rois = spec["K"], spec["rois"]
    N, cap = len(rois), max(rois)
    g = torch.Generator().manual_seed(fill_seed)
    lg = torch.randn((N, cap, K), generator=g)
    rg = torch.randn((N, cap, 4 * K), generator=g)
    pr = torch.rand((N, cap, 4), generator=g) * 100
    pos = 0
    for i, R in enumerate(rois):
        lg[i, :R], rg[i, :R], pr[i, :R] = spec["logits"][pos:pos + R], spec["reg"][pos:pos + R], spec["props"][i]
        pos += R
    counts = torch.tensor(rois, dtype=torch.int32)
    return (lg.reshape(N * cap, K).to(device), rg.reshape(N * cap, 4 * K).to(device), pr.reshape(N * cap, 4).to(device),
            counts.to(device), cap)
