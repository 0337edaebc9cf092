"""Linking a person's tracks across shots, without a GPU: the CPU restatements of ``gcv_face_signature`` and ``gcv_sig_link``
(tests/personutil.py) on rows worked out by hand, ``link_tracks``, and ``scan_frames(persons=True)`` with
``_lib.face_signature`` and ``_lib.sig_link`` replaced by those restatements."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from genconvit_amd import _lib
from genconvit_amd.model import pred_func
from tests import personutil as pu
from tests import scanutil as su

torch.set_grad_enabled(False)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = pu.NONE


def _grey(cells):
    """a 16 x 16 box of one grey pixel per cell: Y = the value, Cb = Cr = 128"""
    img = np.repeat(np.asarray(cells, dtype=np.uint8).reshape(16, 16)[:, :, None], 3, axis=2)
    return pu.signature_of(img, (0, 16, 16, 0)).astype(int)


# ----------------------------------------------------------------------------- the restatement: rows worked out by hand
def test_a_flat_box_is_128_and_its_chroma():
    img = np.zeros((1, 40, 50, 3), dtype=np.uint8)
    img[:] = (10, 200, 30)           # Cb = (32896 - 430 - 17000 + 3840) >> 8 = 75, Cr = (32896 + 1280 - 21400 - 630) >> 8 = 47
    for box in ((0, 0, 50, 40, 0), (0, 3, 47, 20, 30), (0, 24, 16, 40, 0)):
        row = pu.face_signature_ref(img, [box])[0].tolist()
        assert row == [128] * 256 + [75] * 64 + [47] * 64
    assert (pu.face_signature_ref(np.zeros((1, 16, 16, 3), np.uint8), [(0, 0, 16, 16, 0)])[0, :256] == 128).all()


def test_a_two_level_box():
    """the upper half 40, the lower half 200, grey, 32 x 48 pixels: S1 = 128 * 240, d = -+20480, A = 256 * 20480,
    8192 * 20480 / A = 32 exactly (+ 1/2, truncated): 96 above and 160 below whatever the two levels are — gain and offset
    cancel.  Grey has Cb = Cr = 128."""
    for lo, hi in ((40, 200), (0, 255), (100, 101)):
        img = np.full((32, 48, 3), lo, dtype=np.uint8)
        img[16:] = hi
        row = pu.signature_of(img, (0, 48, 32, 0)).tolist()
        assert row == [96] * 128 + [160] * 128 + [128] * 128


def test_rounding_at_one_half():
    """cells 128 + e with e = +64 (126 cells), -64 (126), +63, +65, -63, -65: S1 = 256 * 128, d = 256 e, A = 256 * 16384, so
    (8192 |d| + A / 2) / A = |e| / 2 + 1 / 2 truncated: 63 -> 32 (31.5 goes up, away from 128 on either side), 64 -> 32,
    65 -> 33.  Truncation would give 31, 32, 32."""
    e = [64] * 126 + [-64] * 126 + [63, 65, -63, -65]
    row = _grey([128 + v for v in e])
    assert row[:256].tolist() == [160] * 126 + [96] * 126 + [160, 161, 96, 95]
    assert row[256:].tolist() == [128] * 128


def test_clamping_at_0_and_255():
    """one cell of 255 among 255 of 0: d = 255 * 255 and -255, A = 2 * 255 * 255, so the bright cell is at 128 + 4096 -> 255
    and the others at 128 - (8192 * 255 + 65025) / 130050 = 128 - 16; the inverse clamps at 0"""
    row = _grey([255] + [0] * 255)
    assert row[:256].tolist() == [255] + [112] * 255
    row = _grey([255] * 100 + [0] + [255] * 155)
    assert row[:256].tolist() == [144] * 100 + [0] + [144] * 155


def test_chroma_cells_round_and_stop_at_255():
    """a chroma cell of a 16 x 16 box is 2 x 2 pixels.  (v, v, v + 4) has Cb = (32896 + 512) >> 8 = 130 and Cr =
    (32896 - 84) >> 8 = 128: one such pixel among three greys gives Cb (3 * 128 + 130 + 2) // 4 = 129.  Pure blue has
    Cb = 65536 >> 8 = 256 per pixel, which no byte holds: the cell stops at 255; its Cr = (32896 - 5355) >> 8 = 107.  Pure
    red: Cr 255 and Cb = (32896 - 10965) >> 8 = 85."""
    img = np.full((16, 16, 3), 90, dtype=np.uint8)
    img[5, 6] = (90, 90, 94)                                 # chroma cell (2, 3)
    row = pu.signature_of(img, (0, 16, 16, 0)).astype(int)
    cb = row[256:320].reshape(8, 8)
    assert cb[2, 3] == 129 and (np.delete(cb.reshape(-1), 2 * 8 + 3) == 128).all() and (row[320:] == 128).all()
    blue = np.zeros((20, 16, 3), dtype=np.uint8)
    blue[..., 2] = 255
    assert pu.signature_of(blue, (0, 16, 20, 0))[256:].tolist() == [255] * 64 + [107] * 64
    assert pu.signature_of(blue[..., ::-1], (0, 16, 20, 0))[256:].tolist() == [85] * 64 + [255] * 64


def test_the_8_grid_is_every_other_edge_of_the_16_grid():
    for extent in list(range(16, 300)) + [719, 1080]:
        assert (pu.edges(extent, 8) == pu.edges(extent, 16)[::2]).all()


def test_sig_link_restatement_on_small_cases():
    sig = np.zeros((5, 384), dtype=np.uint8)
    sig[1, :3] = (1, 2, 3)
    sig[2, 0] = 9
    sig[3] = 255
    sig[4, 383] = 200
    d = pu.sig_link_ref(sig, [0, 1, 1, 2, -1], 4)
    assert d.tolist() == [[NONE, 6, 97920, NONE], [6, NONE, 97920 - 9, NONE], [97920, 97911, NONE, NONE], [NONE] * 4]
    assert pu.sig_link_ref(sig[:0], [], 2).tolist() == [[NONE, NONE], [NONE, NONE]]
    assert pu.sig_link_ref(sig, [0] * 5, 1).tolist() == [[NONE]] and pu.sig_link_ref(sig[:0], [], 0).shape == (0, 0)


def test_the_default_link_max_is_midway_on_the_synthetic_identities():
    same, other = pu.identity_distances()
    assert (same, other) == (5804, 12361)
    assert pred_func.PERSON_DEFAULTS["link_max"] == (same + other) // 2 == 9082
    for text in (pred_func.link_tracks.__doc__, pred_func.scan_frames.__doc__,
                 open(os.path.join(REPO, "DESIGN.md")).read()):
        assert "5 804" in text and "12 361" in text and "9 082" in text


# ----------------------------------------------------------------------------- link_tracks
def _tracks(*frames):
    return [[(f, 0, 20, 20, 0) for f in fs] for fs in frames]


def _dist(T, pairs):
    d = np.full((T, T), NONE, dtype=np.int64)
    for (a, b), v in pairs.items():
        d[a, b] = d[b, a] = v
    return d


def test_link_tracks_joins_below_the_threshold():
    tr = _tracks([0, 1], [2, 3], [4, 5], [6, 7])
    d = _dist(4, {(0, 2): 100, (1, 3): 200, (0, 1): 900, (2, 3): 901, (0, 3): 902, (1, 2): 903})
    assert pred_func.link_tracks(d, tr, 500) == [[0, 2], [1, 3]]
    assert pred_func.link_tracks(d, tr, 99) == [[0], [1], [2], [3]]
    assert pred_func.link_tracks(d, tr, 100) == [[0, 2], [1], [3]]                          # <=, not <
    assert pred_func.link_tracks(d, tr, 900) == [[0, 1, 2, 3]]
    assert pred_func.link_tracks(torch.as_tensor(d), tr, 500) == [[0, 2], [1, 3]]
    assert pred_func.link_tracks(d, tr) == pred_func.link_tracks(d, tr, pred_func.PERSON_DEFAULTS["link_max"])


def test_link_tracks_takes_ties_in_track_order():
    """tracks 0 and 1 share frame 0; track 2 is as close to the one as to the other: (5, 0, 2) comes before (5, 1, 2), so 2
    goes to 0, and the pair (1, 2) is then vetoed"""
    tr = _tracks([0, 1], [0, 1], [5, 6])
    assert pred_func.link_tracks(_dist(3, {(0, 2): 5, (1, 2): 5, (0, 1): 5}), tr, 10) == [[0, 2], [1]]
    assert pred_func.link_tracks(_dist(3, {(0, 2): 5, (1, 2): 4, (0, 1): 5}), tr, 10) == [[0], [1, 2]]


def test_link_tracks_vetoes_a_shared_frame_also_after_a_union():
    tr = _tracks([0, 1, 2], [2, 3], [10, 11], [3, 12])
    assert pred_func.link_tracks(_dist(4, {(0, 1): 0}), tr, 10) == [[0], [1], [2], [3]]     # frame 2 is in both
    # 0-2 and 1-3 join first; 2-3 would be fine by the tracks themselves (frames 10, 11 against 3, 12), but their clusters
    # hold tracks 0 and 1, which share frame 2
    d = _dist(4, {(0, 2): 1, (1, 3): 2, (2, 3): 3})
    assert pred_func.link_tracks(d, _tracks([0, 1, 2], [2, 4], [10, 11], [12, 13]), 10) == [[0, 2], [1, 3]]
    assert pred_func.link_tracks(d, _tracks([0, 1], [2, 4], [10, 11], [12, 13]), 10) == [[0, 1, 2, 3]]


def test_link_tracks_never_links_an_unmeasured_pair_and_small_inputs():
    tr = _tracks([0], [1])
    assert pred_func.link_tracks(_dist(2, {}), tr, NONE) == [[0], [1]]
    assert pred_func.link_tracks(_dist(2, {}), tr, float(2 ** 40)) == [[0], [1]]
    assert pred_func.link_tracks(np.empty((0, 0)), [], 10) == []
    assert pred_func.link_tracks([[NONE]], _tracks([3]), 10) == [[0]]
    for bad in (dict(link_max=-1), dict(link_max=None), dict(link_max=True), dict(link_max=float("nan"))):
        with pytest.raises(ValueError):
            pred_func.link_tracks(_dist(2, {}), tr, **bad)
    with pytest.raises(ValueError):
        pred_func.link_tracks(_dist(3, {}), tr, 10)


def test_the_defaults_are_stated_once():
    seen = set()
    for f in (pred_func.link_tracks, pred_func._check_persons):
        sig = inspect.signature(f).parameters
        assert [k for k in pred_func.PERSON_DEFAULTS if k in sig], f
        assert all(sig[k].default == v for k, v in pred_func.PERSON_DEFAULTS.items() if k in sig), f
        seen |= set(sig) & set(pred_func.PERSON_DEFAULTS)
    assert seen == set(pred_func.PERSON_DEFAULTS) == {"link_max", "per_track"}
    src = inspect.getsource(pred_func)
    assert len(re.findall(r"link_max=\d", src)) == 1 and len(re.findall(r"per_track=\d", src)) == 1      # the dict itself


# ----------------------------------------------------------------------------- face_signatures, scan_frames(persons=True)
@pytest.fixture
def spy(monkeypatch):
    """``_lib.face_signature`` and ``_lib.sig_link`` are the restatements behind the bindings' own checks; every call is
    recorded: ("sig", frames of the slab, rows) and ("link", n, owner, T)"""
    calls = []

    def face_signature(frames_u8, boxes):
        boxes = [tuple(int(v) for v in b) for b in boxes]
        calls.append(("sig", frames_u8.shape[0], boxes))
        _lib._check_quality_boxes("face_signature", boxes, *frames_u8.shape[:3], 16)
        return torch.as_tensor(pu.face_signature_ref(frames_u8, boxes))

    def sig_link(sig, owner, tracks):
        o, tracks = _lib._check_sig_link("sig_link", sig, owner, tracks)
        calls.append(("link", sig.shape[0], o.tolist(), tracks))
        return torch.as_tensor(pu.sig_link_ref(sig, o.numpy(), tracks))
    monkeypatch.setattr(_lib, "face_signature", face_signature)
    monkeypatch.setattr(_lib, "sig_link", sig_link)
    return calls


class StandIn(torch.nn.Module):
    """logits = (k m, -k m) with m the crop's mean normalised red (the stand-in of tests/test_scan_cpu.py, one network)"""
    net = "ed"

    def __init__(self):
        super().__init__()
        self.k = torch.nn.Parameter(torch.tensor(4.0))

    def forward(self, x, eps=None):
        m = x[:, 0].float().mean((1, 2))
        return torch.stack((self.k * m, -self.k * m), 1)


@pytest.fixture
def on_cpu(monkeypatch):
    votes = []
    monkeypatch.setattr(_lib, "face_crop_preprocess", lambda frames_u8, boxes, size=224, dtype=None:
                        su.face_crop_preprocess_ref(frames_u8, boxes, size, dtype))

    def vote_windows(logits, batch, nets, ranges):
        votes.append((logits.clone(), batch, nets, list(ranges)))
        frame_p, mean2 = su.vote_windows_ref(logits, batch, nets, ranges)
        return frame_p.float(), mean2.float()
    monkeypatch.setattr(_lib, "vote_windows", vote_windows)
    return votes


PLAIN_KEYS = ["boxes", "frame_scores", "segments", "track_offsets", "track_verdicts", "tracks", "verdict", "window_means",
              "windows"]
PERSON_KEYS = ["distance", "means", "measured", "of_track", "rows", "tracks", "verdicts"]


def test_face_signatures_groups_host_frames_and_skips_small_boxes(spy):
    frames = np.random.default_rng(12).integers(0, 256, (5, 60, 80, 3), dtype=np.uint8)
    boxes = [(4, 0, 80, 60, 0), (0, 5, 40, 30, 10), (2, 10, 25, 40, 10), (4, 20, 50, 50, 10), (1, 1, 30, 16, 3),
             (0, 30, 80, 60, 40), (2, 0, 17, 16, 0)]                                       # box 2 is 15 wide, box 4 15 high
    big = [0, 1, 3, 5, 6]
    got = pred_func.face_signatures(frames, boxes, dev="cpu")
    assert sorted(got) == ["measured", "sig"] and got["measured"].tolist() == [i in big for i in range(7)]
    assert got["sig"].dtype == torch.uint8 and tuple(got["sig"].shape) == (7, 384)
    assert (got["sig"][big].numpy() == pu.face_signature_ref(frames, [boxes[i] for i in big])).all()
    assert not got["sig"][[2, 4]].any()
    assert [c[1] for c in spy] == [3] and spy[0][2][0] == (0, *boxes[1][1:])               # frames 0, 2, 4 in one slab
    for max_frames, slabs in ((1, [1, 1, 1]), (2, [2, 1])):
        del spy[:]
        again = pred_func.face_signatures(torch.as_tensor(frames), boxes, max_frames=max_frames, dev="cpu")
        assert [c[1] for c in spy] == slabs and torch.equal(again["sig"], got["sig"])
    del spy[:]
    none = pred_func.face_signatures(frames, [], dev="cpu")
    assert tuple(none["sig"].shape) == (0, 384) and none["measured"].shape == (0,)
    small = pred_func.face_signatures(frames, [boxes[2], boxes[4]], dev="cpu")
    assert not small["measured"].any() and not small["sig"].any() and spy == []
    with pytest.raises(ValueError):
        pred_func.face_signatures(frames, boxes, max_frames=0)
    with pytest.raises(_lib.GenConViTHipError):
        pred_func.face_signatures(frames, [(0, 0, 81, 60, 0)])
    with pytest.raises(_lib.GenConViTHipError):
        pred_func.face_signatures(frames.astype(np.float32), boxes)
    assert spy == []


def test_scan_frames_without_persons_is_unchanged(spy, on_cpu):
    frames, det, cuts = pu.interview()
    for kw in ({}, dict(persons=None), dict(persons=False), dict(persons=None, person_args=dict(nonsense=1))):
        res = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, cuts=cuts, **kw)
        assert sorted(res) == sorted(PLAIN_KEYS + ["cuts"]) and len(res["tracks"]) == 4
    assert spy == [] and len(on_cpu) == 4


def test_scan_frames_finds_the_two_speakers_of_an_interview(spy, on_cpu):
    frames, det, cuts = pu.interview()
    plain = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, cuts=cuts)
    del on_cpu[:]
    res = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, cuts=cuts, persons=True)
    assert sorted(res) == sorted(PLAIN_KEYS + ["cuts", "persons"])
    for key in PLAIN_KEYS + ["cuts"]:
        same = torch.equal(res[key], plain[key]) if torch.is_tensor(res[key]) else res[key] == plain[key]
        assert same, key
    p = res["persons"]
    assert sorted(p) == PERSON_KEYS
    assert p["tracks"] == [[0, 2], [1, 3]] and p["of_track"] == [0, 1, 0, 1]
    assert p["rows"] == list(range(16)) and p["measured"].all() and p["measured"].dtype == bool
    want = pu.sig_link_ref(pu.face_signature_ref(frames, res["boxes"]), [t for t in range(4) for _ in range(4)], 4)
    assert p["distance"].dtype == np.int64 and (p["distance"] == want).all()
    link_max = pred_func.PERSON_DEFAULTS["link_max"]
    assert max(want[0, 2], want[1, 3]) <= link_max < min(want[0, 1], want[0, 3], want[1, 2], want[2, 3])
    # one launch for the signatures of all 16 rows (the frames are few enough for one slab), one link
    assert [c[0] for c in spy] == ["sig", "link"] and spy[0][1] == 16 and spy[1][1:] == (16, [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4, 4)
    # the second vote: the logits of person 0's rows (tracks 0 and 2), then person 1's; each person's rows one range
    assert len(on_cpu) == 2
    first, second = on_cpu
    order = [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]
    assert torch.equal(second[0], first[0][order]) and second[1:] == (16, 1, [(0, 8), (8, 16)])
    fp = res["frame_scores"].double()
    assert tuple(p["means"].shape) == (2, 2) and p["means"].dtype == torch.float32
    for k, rows in enumerate(([0, 1, 2, 3, 8, 9, 10, 11], [4, 5, 6, 7, 12, 13, 14, 15])):
        assert (p["means"][k].double() - fp[rows].mean(0)).abs().max().item() <= 1e-6
        assert p["verdicts"][k] == pred_func._verdict(p["means"][k].cpu())
    # nothing links at link_max = 0: four persons, each with its track's verdict
    alone = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, cuts=cuts, persons=True, person_args=dict(link_max=0))
    assert alone["persons"]["tracks"] == [[0], [1], [2], [3]] and alone["persons"]["verdicts"] == alone["track_verdicts"]
    # and without the cuts position makes one track of the four shots: one person
    one = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, iou=0.2, persons=True)
    assert len(one["tracks"]) == 1 and one["persons"]["tracks"] == [[0]] and one["persons"]["distance"].tolist() == [[NONE]]
    assert one["persons"]["verdicts"] == [one["verdict"]]


def test_scan_frames_samples_per_track_rows_evenly(spy, on_cpu):
    frames, det, cuts = pu.interview()
    res = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, cuts=[4], persons=True, person_args=dict(per_track=5))
    assert [len(t) for t in res["tracks"]] == [4, 12]
    # track 0: all 4 rows; track 1 (rows 4 ... 15): (k * 12) // 5 = 0, 2, 4, 7, 9
    assert res["persons"]["rows"] == [0, 1, 2, 3, 4, 6, 8, 11, 13]
    # only the nine frames with a sampled row go up, and the rows count frames within that slab
    sampled = [res["boxes"][i] for i in res["persons"]["rows"]]
    assert spy[0][1] == 9 and spy[0][2] == [(k, *b[1:]) for k, b in enumerate(sampled)]
    assert spy[1][1:] == (9, [0] * 4 + [1] * 5, 2)
    one = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, cuts=[4], persons=True, person_args=dict(per_track=1))
    assert one["persons"]["rows"] == [0, 4]
    # host frames go up in slabs of at most max_batch frames for this pass too
    del spy[:]
    pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, cuts=[4], max_batch=4, persons=True)
    assert [c[1] for c in spy if c[0] == "sig"] == [4, 4, 4, 4]


def test_scan_frames_never_joins_two_faces_of_the_same_frames(spy, on_cpu):
    frames, det = pu.twins()
    res = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, persons=True)
    p = res["persons"]
    assert len(res["tracks"]) == 2 and p["distance"][0, 1] < 1000 < pred_func.PERSON_DEFAULTS["link_max"]
    assert p["tracks"] == [[0], [1]] and p["of_track"] == [0, 1] and p["verdicts"] == res["track_verdicts"]
    far = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, persons=True, person_args=dict(link_max=97920))
    assert far["persons"]["tracks"] == [[0], [1]]


def test_scan_frames_persons_without_a_face(spy, on_cpu):
    frames, _, cuts = pu.interview()
    res = pred_func.scan_frames(frames, StandIn(), boxes=[], cuts=cuts, persons=True)
    p = res["persons"]
    assert res["verdict"] == (None, None) and spy == [] and on_cpu == [] and sorted(p) == PERSON_KEYS
    assert p["tracks"] == [] and p["of_track"] == [] and p["verdicts"] == [] and p["rows"] == []
    assert p["distance"].shape == (0, 0) and tuple(p["means"].shape) == (0, 2) and p["measured"].shape == (0,)


def test_scan_frames_samples_only_rows_the_quality_gate_kept(spy, on_cpu, monkeypatch):
    """frames 5 and 6 (shot 1) are painted black inside the face box: ``quality=True`` drops those rows, and the signatures
    are taken from the rows that remain — the dropped boxes are never described"""
    from tests import qualityutil as qu
    monkeypatch.setattr(_lib, "face_quality", lambda frames_u8, boxes, grid=64: torch.as_tensor(
        qu.face_quality_ref(frames_u8, [tuple(int(v) for v in b) for b in boxes], grid)))
    frames, det, cuts = pu.interview()
    for f in (5, 6):
        _, top, right, bottom, left = det[f]
        frames[f, top:bottom, left:right] = 0
    res = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, cuts=cuts, quality=True, quality_args=dict(grid=16),
                                persons=True)
    assert np.nonzero(~res["quality"]["kept"])[0].tolist() == [5, 6] and len(res["boxes"]) == 14
    assert res["track_offsets"] == [0, 4, 6, 10, 14] and res["persons"]["rows"] == list(range(14))
    slab, described = [c for c in spy if c[0] == "sig"][0][1:]
    assert slab == 14 and described == [(k, *b[1:]) for k, b in enumerate(res["boxes"])]   # frames 5 and 6 do not even go up
    assert det[5] not in res["boxes"] and det[6] not in res["boxes"]
    assert res["persons"]["tracks"] == [[0, 2], [1, 3]]


def test_scan_frames_leaves_a_small_face_unmeasured_and_alone(spy, on_cpu):
    frames, det, cuts = pu.interview()
    det = det[:12] + [(f, 30, 55, 45, 40) for f in range(12, 16)]                          # the last shot's boxes: 15 x 15
    res = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, cuts=cuts, persons=True)
    p = res["persons"]
    assert p["measured"].tolist() == [True] * 12 + [False] * 4 and spy[1][2][12:] == [-1] * 4
    assert (p["distance"][3] == NONE).all() and (p["distance"][:, 3] == NONE).all()
    assert p["tracks"] == [[0, 2], [1], [3]] and p["of_track"] == [0, 1, 0, 2]


def test_scan_frames_refuses_bad_person_arguments_before_anything_runs(spy, on_cpu, monkeypatch):
    frames, det, cuts = pu.interview()
    monkeypatch.setattr(pred_func, "track_boxes", lambda *a, **k: pytest.fail("ran"))
    for bad in (dict(person_args=dict(link_max=-1)), dict(person_args=dict(per_track=0)), dict(person_args=dict(per_track=2.5)),
                dict(person_args=dict(per_track=True)), dict(person_args=[("link_max", 5)]), dict(person_args=dict(grid=16)),
                dict(person_args=dict(link_max="far")), dict(persons="yes"), dict(persons=1)):
        with pytest.raises(ValueError):
            pred_func.scan_frames(frames, StandIn(), boxes=det, cuts=cuts, **{"persons": True, **bad})
    assert spy == [] and on_cpu == []


# ----------------------------------------------------------------------------- the bindings' refusals
def test_the_bindings_refuse_before_any_launch(monkeypatch):
    """none of these reaches the library: a launch without a GPU would fail differently"""
    monkeypatch.setattr(_lib, "check", lambda *a, **k: pytest.fail("launched"))
    frames = torch.zeros((2, 60, 80, 3), dtype=torch.uint8)
    with pytest.raises(_lib.GenConViTHipError, match="device tensor"):
        _lib.face_signature(frames, [(0, 0, 40, 40, 0)])
    sig = torch.zeros((4, 384), dtype=torch.uint8)
    with pytest.raises(_lib.GenConViTHipError, match="device tensor"):
        _lib.sig_link(sig, [0, 1, 1, 0], 2)
    check = lambda s=sig, o=(0, 1, -1, 0), t=2: _lib._check_sig_link("t", s, o, t)
    o, t = check()
    assert o.tolist() == [0, 1, -1, 0] and o.dtype == torch.int32 and t == 2
    for kw in (dict(o=(0, 1, 2, 0)), dict(o=(0, 1, -2, 0)), dict(o=(0, 1, 0)), dict(t=-1), dict(t=4097), dict(t=True),
               dict(s=sig[:, :383]), dict(s=sig.float()), dict(s=sig.numpy()), dict(s=sig.reshape(2, 2, 384))):
        with pytest.raises(_lib.GenConViTHipError):
            check(**kw)
    with pytest.raises(_lib.GenConViTHipError, match="at most 65536"):
        _lib._check_sig_link("t", torch.zeros((65537, 384), dtype=torch.uint8), [0] * 65537, 1)
    check(t=4096)


def test_the_header_declares_both_entries_and_states_their_arithmetic():
    hdr = open(os.path.join(REPO, "include", "genconvit_hip.h")).read()
    assert re.search(r"int gcv_face_signature\(const void\* frames_u8_nhwc, int nframes, int H, int W, const int\* boxes5, "
                     r"int n, void\* sig384,\s+gcv_stream stream\);", hdr)
    assert re.search(r"int gcv_sig_link\(const void\* sig384, const int\* owner, int n, int tracks, uint32_t\* out_u32, "
                     r"gcv_stream stream\);", hdr)
    assert len(_lib.SIGNATURES["gcv_face_signature"][1]) == 8 and len(_lib.SIGNATURES["gcv_sig_link"][1]) == 6
    for word in ("(i h) >> 4", "(i h) >> 3", "8192 |d| + A // 2", "32896 - 43 R - 85 G + 128 B", "32896 + 128 R - 107 G - 21 B",
                 "0xFFFFFFFF", "97 920", "tests/personutil.py"):
        assert word in hdr, word
