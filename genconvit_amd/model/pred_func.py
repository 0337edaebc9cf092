"""Inference API — mirror of the reference's ``model/pred_func.py:18-184`` for the hot path.

Same names and argument meaning (``load_genconvit``, ``preprocess_frame``, ``pred_vid``,
``max_prediction_value``, ``real_or_fake``, ``df_face``, ``face_rec``, ``extract_frames``,
``is_video``, ``set_result``, ``store_result``), plus what the reference lacks: evidence maps (``explain_*``) and the
whole-video scan with per-track sliding-window verdicts (``scan_frames``, ``scan_video``; ``follow_tracks`` moves the
boxes of frames the detector skipped onto the face, ``shot_cuts`` finds the hard cuts at which tracks end, ``shot_transitions`` the fades and dissolves whose frames stay out
of them; ``render_scan`` / ``render_video`` draw the scan's result back onto the frames; ``YUV420`` / ``read_yuv420`` hand all of
these a decoder's YUV 4:2:0 frames in place of RGB).  ``prediction.py`` star-imports this module and
relies on ``torch``/``os``/``np`` coming along, so they stay module globals.  The heavy CPU-side
dependencies (dlib, face_recognition, decord) are imported lazily inside the video / face
functions so the model path imports on a box without them; cv2 is not needed any more (the crop +
INTER_AREA resize of ``face_rec`` runs on the device, row N4).
"""
import collections
import os

import numpy as np
import torch

from .. import _lib, synth
from .config import load_config
from .genconvit import GenConViT, normalize_cams

device = "cuda" if torch.cuda.is_available() else "cpu"


def load_genconvit(config, net, ed_weight, vae_weight, fp16, arch_type="original", use_attention=True,
                   use_residual=True):
    """reference model/pred_func.py:18-64.  ``arch_type='v2'`` (an experiment fork with a different,
    incompatible architecture) is out of scope of this build and rejected explicitly."""
    device_str = "cuda" if torch.cuda.is_available() else "cpu"
    print(f"Using device: {device_str}")
    if arch_type == "v2":
        raise NotImplementedError("GenConViTV2 is an experiment fork outside this build's scope (SURVEY.md §2 #9)")
    model = GenConViT(config, ed=ed_weight, vae=vae_weight, net=net, fp16=fp16)
    model.to(device)
    model.eval()
    if fp16:
        model.half()
    return model


_MEAN = torch.tensor(synth.IMAGENET_MEAN, dtype=torch.float32).view(1, 3, 1, 1)
_STD = torch.tensor(synth.IMAGENET_STD, dtype=torch.float32).view(1, 3, 1, 1)


def preprocess_frame(frame):
    """uint8 (N,224,224,3) -> normalised fp32 NCHW (reference :95-108 with the 'vid' transform of
    dataset/loader.py:63-65,77), vectorised over the batch instead of a per-frame Python loop."""
    u8 = frame if torch.is_tensor(frame) else torch.as_tensor(np.asarray(frame))
    if torch.cuda.is_available() and u8.dtype == torch.uint8:
        # row N1: ship the uint8 crops (4x fewer H2D bytes than fp32) and normalise on the device
        return _lib.preprocess(u8.to(device))
    df_tensor = u8.float().permute((0, 3, 1, 2)) / 255.0
    return (df_tensor - _MEAN) / _STD


def pred_vid(df, model):
    """reference :111-120: sigmoid over logits, mean over rows, argmax."""
    with torch.no_grad():
        p = next(model.parameters())
        if df.device != p.device:
            df = df.to(p.device)
        return max_prediction_value(torch.sigmoid(model(df).squeeze()))


def pred_vid_explain(df, model, target=None, layer="s3"):
    """``pred_vid`` with evidence maps: returns ``((y, y_val), maps)`` where ``(y, y_val)`` is what ``pred_vid(df, model)``
    returns for the same logits and ``maps`` is the model's per-frame Grad-CAM maps upsampled to 224 x 224 and scaled to
    [0, 1] per map, in the logits' row order ((2n, 224, 224) for the ensemble: ED rows, then VAE rows).  ``target``: as in
    ``GenConViT.explain`` (default: each frame's own decision); ``layer``: "s3" (7 x 7 maps of the last ConvNeXt stage) or
    "s2" (14 x 14 maps of the stage before it), as in ``GenConViT.explain``."""
    p = next(model.parameters())
    if df.device != p.device:
        df = df.to(p.device)
    logits, cams = model.explain(df, target=target, upsample=True, layer=layer)
    out = logits.to(p.dtype) if getattr(model, "reference_logits_dtype", False) else logits
    return max_prediction_value(torch.sigmoid(out.squeeze())), normalize_cams(cams["upsampled"])


def pred_vids(dfs, model, max_batch=128):
    """Row N3: the reference calls the model once per video with <= 15 frames
    (prediction.py:231-266); here the face crops of MANY videos are concatenated into batches of up to
    ``max_batch`` frames, run through one forward each, and voted per video on the device.  Returns
    ``[(y, y_val), ...]`` with the exact ``pred_vid`` semantics per video."""
    results = [None] * len(dfs)
    order = [i for i, d in enumerate(dfs) if len(d) >= 1]
    p = next(model.parameters())
    nets = 2 if getattr(model, "net", "genconvit") not in ("ed", "vae") else 1
    i = 0
    with torch.no_grad():
        while i < len(order):
            group, n = [], 0
            while i < len(order) and (not group or n + len(dfs[order[i]]) <= max_batch):
                group.append(order[i])
                n += len(dfs[order[i]])
                i += 1
            batch = torch.cat([dfs[g].to(p.device) for g in group])
            offs = torch.tensor([0] + list(np.cumsum([len(dfs[g]) for g in group])), dtype=torch.int32)
            logits = model(batch)
            means = _lib.vote_segments(logits, batch.shape[0], nets, offs).cpu()
            for k, g in enumerate(group):
                m = means[k]
                results[g] = (int(torch.argmax(m).item()),
                              m[0].item() if m[0] > m[1] else abs(1 - m[1]).item())
    return results


def max_prediction_value(y_pred):
    """reference :123-131 (the device-side reduction is ``genconvit_amd._lib.vote``)."""
    mean_val = torch.mean(y_pred, dim=0)
    return (
        torch.argmax(mean_val).item(),
        mean_val[0].item() if mean_val[0] > mean_val[1] else abs(1 - mean_val[1]).item(),
    )


def real_or_fake(prediction):
    return {0: "REAL", 1: "FAKE"}[prediction ^ 1]


def extract_frames(video_file, frames_nums=15):
    from decord import VideoReader, cpu
    vr = VideoReader(video_file, ctx=cpu(0))
    step_size = max(1, len(vr) // frames_nums)
    return vr.get_batch(list(range(0, len(vr), step_size))[:frames_nums]).asnumpy()


def face_locations(frames, keep_all=False):
    """The detector call of the reference's face_rec (:71-76): dlib's CNN / HOG detector through ``face_recognition``
    on the CPU (third-party; imported lazily).  Returns rows (frame index, top, right, bottom, left), at most
    ``len(frames)`` of them in frame order — the reference stops filling ``temp_face`` there (:78,88-89).
    ``keep_all=True`` lifts that cut and returns every face of every frame (``scan_frames``)."""
    import dlib
    import face_recognition
    mod = "cnn" if dlib.DLIB_USE_CUDA else "hog"
    boxes = []
    for i, frame in enumerate(frames):
        bgr = np.ascontiguousarray(frame[..., ::-1])          # cv2.cvtColor(frame, cv2.COLOR_RGB2BGR) (:72)
        for loc in face_recognition.face_locations(bgr, number_of_times_to_upsample=0, model=mod):
            if keep_all or len(boxes) < len(frames):
                boxes.append((i, *loc))
    return boxes


def crop_faces(frames, boxes, size=224):
    """Row N4: crop + ``cv2.INTER_AREA`` resize of every box on the MI355X (``gcv_face_crop_resize``); the RGB<->BGR
    swaps the reference wraps around the resize (:72,86) cancel.  uint8 (n,size,size,3) on the device."""
    fr = frames if torch.is_tensor(frames) else torch.as_tensor(np.ascontiguousarray(frames))
    return _lib.face_crop_resize(fr.to(device), boxes, size)


def face_rec(frames, p=None, klass=None, locate=None):
    """reference :67-92.  Detection stays third-party CPU code (``locate``, default ``face_locations`` above); the crops
    are cut and resized on the device and come back as the uint8 array the reference returns."""
    boxes = (locate or face_locations)(frames)
    if len(boxes) == 0:
        return [], 0
    boxes = boxes[:len(frames)]
    return crop_faces(frames, boxes).cpu().numpy(), len(boxes)


def _overlay_maps(model, cams, which):
    """The map ``explain_frames`` draws for each face, (n, side, side) fp32 in [0, 1]: the original-frame pass of the ED,
    the backbone(x) map of the VAE, or for the ensemble the one ``which`` names ("mean": the mean of the two after each
    is scaled to [0, 1], not rescaled again)."""
    net = getattr(model, "net", "genconvit")
    ed = lambda: normalize_cams(cams["ed"][:, 1])
    vae = lambda: normalize_cams(cams["vae"])
    if net in ("ed", "vae"):
        return ed() if net == "ed" else vae()
    return ed() if which == "ed" else vae() if which == "vae" else (ed() + vae()) * 0.5


def explain_frames(frames, model, boxes=None, locate=None, eps=None, target=None, layer="s3", which="mean", alpha=0.5,
                   weighted=True, lut=None):
    """The verdict on the faces of ``frames`` with the evidence drawn over them: returns ``((y, y_val), overlays, boxes)``.
    ``frames``: uint8 (F,H,W,3) RGB, numpy or tensor; ``boxes``: rows (frame index, top, right, bottom, left) — by default
    what ``(locate or face_locations)(frames)`` finds —, cut at ``len(frames)`` rows as ``face_rec`` does.  The faces are
    cropped and normalised on the device (``crop_faces``, ``preprocess_frame``) and run through ``model.explain`` (``eps``,
    ``target``, ``layer`` as there; the 224-pixel upsampling is skipped); ``(y, y_val)`` is what ``pred_vid_explain`` returns
    for those crops.  Each face's map (``which``: "ed", "vae" or "mean" for the ensemble; a single network draws its own),
    scaled to [0, 1], is drawn over its box as a colour heat overlay (``_lib.cam_overlay``: ``alpha``, ``weighted``,
    ``lut``), sampled from the raw 7 x 7 / 14 x 14 cells at the box's own size and aspect.  ``overlays``: uint8 (F,H,W,3)
    on the device; ``boxes``: the list used.  No face: ``((None, None), the frames on the device, [])``, nothing is run."""
    if which not in ("ed", "vae", "mean"):
        raise ValueError(f"unknown map {which!r}: accepted values are 'ed', 'vae' and 'mean'")
    fr = _as_frames("explain_frames", frames)
    if boxes is None:
        boxes = (locate or face_locations)(fr.rgb(None, device).cpu().numpy() if isinstance(fr, YUV420) else frames)
    boxes = list(boxes)[:len(fr)]
    _lib._check_boxes("explain_frames", boxes, *fr.shape[:3])
    fr = _rgb_slab(fr, slice(None), device)
    if len(boxes) == 0:
        return (None, None), fr, []
    df = preprocess_frame(crop_faces(fr, boxes))
    p = next(model.parameters())
    if df.device != p.device:
        df = df.to(p.device)
    logits, cams = model.explain(df, eps=eps, target=target, upsample=False, layer=layer)
    out = logits.to(p.dtype) if getattr(model, "reference_logits_dtype", False) else logits
    verdict = max_prediction_value(torch.sigmoid(out.squeeze()))
    return verdict, _lib.cam_overlay(fr, boxes, _overlay_maps(model, cams, which), alpha, weighted, lut), boxes


def explain_video(vid, model, num_frames=15, **kw):
    """``explain_frames`` on ``num_frames`` frames of the video file ``vid`` (``extract_frames``)."""
    return explain_frames(extract_frames(vid, num_frames), model, **kw)


def window_ranges(length, window, stride):
    """The sliding windows over a track of ``length`` frames as ``[(lo, hi), ...]``: none for ``length <= 0``, the whole
    track for ``length <= window``, else the starts 0, stride, 2 stride, ... while the window fits, plus a last window
    ending at ``length`` when the stride does not land there — the tail of a track is always covered."""
    if window < 1 or stride < 1:
        raise ValueError(f"window_ranges: window {window} and stride {stride} must both be at least 1")
    if length <= 0:
        return []
    if length <= window:
        return [(0, length)]
    starts = list(range(0, length - window + 1, stride))
    if starts[-1] != length - window:
        starts.append(length - window)
    return [(s, s + window) for s in starts]


class YUV420:
    """Frames as a video decoder delivers them — YUV 4:2:0, 1.5 bytes a pixel — for everything here that takes RGB frames:
    ``scan_frames``, ``follow_tracks``, ``extend_tracks``, ``shot_cuts``, ``shot_transitions``, ``face_quality``,
    ``face_signatures``, ``explain_frames`` and ``render_scan`` accept a ``YUV420`` where they accept uint8 (F,H,W,3) RGB.
    ``data``: uint8 (F, 3H/2, W), numpy or a tensor on either device, one row of 3HW/2 bytes per frame, H and W even;
    ``layout``: "i420" (the Y plane, then U, then V, what ``-pix_fmt yuv420p -f rawvideo`` writes) or "nv12" (the Y plane,
    then rows of interleaved U, V: a hardware decoder's surface); ``matrix``: "bt601" or "bt709"; ``full_range``: 0 ... 255
    rather than Y 16 ... 235, C 16 ... 240.  Anything else is a ``GenConViTHipError`` here, before anything runs.
    A stage asks for the frames of one of its groups and gets them as RGB on the device (``rgb``): host bytes are
    uploaded as YUV, half of what RGB frames weigh, and one ``_lib.yuv420_to_rgb`` launch converts the group (include/
    genconvit_hip.h states the integer arithmetic; each chroma sample serves its 2 x 2 block).  The groups are the ones
    host RGB frames are cut into — also for data already on the device, whose RGB form never exists as a whole — so
    every later launch sees the slab and the batch it would see for the same pixels given as RGB.
    ``shape`` is the RGB shape (F, H, W, 3); ``len``, ``is_cuda`` and ``device`` describe ``data``."""

    def __init__(self, data, layout="i420", matrix="bt709", full_range=False):
        t = data if torch.is_tensor(data) else torch.as_tensor(np.ascontiguousarray(data))
        if not (t.dtype == torch.uint8 and t.dim() == 3):
            raise _lib.GenConViTHipError("YUV420: data must be uint8 of shape (F, 3H/2, W)")
        nf, h, w = _lib.yuv420_geometry("YUV420", t.shape)
        _lib._check_yuv_names("YUV420", layout, matrix)
        self.data, self.layout, self.matrix, self.full_range = t.contiguous(), layout, matrix, bool(full_range)
        self.shape = (nf, h, w, 3)

    def __len__(self):
        return self.shape[0]

    @property
    def is_cuda(self):
        return self.data.is_cuda

    @property
    def device(self):
        return self.data.device

    @property
    def colour(self):
        return {"matrix": self.matrix, "full_range": self.full_range}

    def rgb(self, index=None, dev=None):
        """The frames ``index`` (None: all; a slice; a list of frame numbers) as a uint8 (n,H,W,3) RGB slab on the device:
        their bytes go to ``dev`` (default: where they are if that is a GPU, else this module's ``device``) and one
        ``_lib.yuv420_to_rgb`` converts them.  The slab is new with every call."""
        d = self.data
        if isinstance(index, slice):
            d = d[index]
        elif index is not None:
            d = d.index_select(0, torch.as_tensor(index, dtype=torch.int64, device=d.device))
        return _lib.yuv420_to_rgb(d.to(dev if dev is not None else d.device if d.is_cuda else device), self.layout, self.matrix,
                                  self.full_range)


def _as_frames(what, frames):
    """``frames`` (numpy or a tensor on either device) as a tensor; anything but uint8 (F,H,W,3) is an error.  A ``YUV420``
    passes through: it has the shape, and ``_rgb_slab`` gets its pixels."""
    if isinstance(frames, YUV420):
        return frames
    fr = frames if torch.is_tensor(frames) else torch.as_tensor(np.ascontiguousarray(frames))
    if not (fr.dtype == torch.uint8 and fr.dim() == 4 and fr.shape[3] == 3):
        raise _lib.GenConViTHipError(f"{what}: frames must be uint8 of shape (F,H,W,3)")
    return fr


def _resident(fr):
    """Are the frames RGB on a GPU, to be used in place?  Host frames and every ``YUV420`` go group by group."""
    return torch.is_tensor(fr) and fr.is_cuda


def _rgb_slab(fr, index, dev, copy=False):
    """The frames ``index`` (a slice or a sorted list of frame numbers) of ``fr`` as an RGB slab on ``dev``: the one place
    where a stage's group of frames reaches the device, uploaded as they are, or as YUV and converted there.  ``copy``: the
    slab is the caller's to draw on even when the frames are on ``dev`` already."""
    if isinstance(fr, YUV420):
        return fr.rgb(index, dev)
    if isinstance(index, slice):
        return fr[index].to(dev, copy=True) if copy else fr[index].to(dev)
    return fr.index_select(0, torch.as_tensor(index, device=fr.device)).to(dev)


def _upload(fr, used, dev):
    """What one group of a stage needs of ``fr``: the frames ``used`` (frame numbers, sorted) as a slab on ``dev``, and the map
    from frame number to slab row.  Which rows make a group is each stage's own business."""
    return _rgb_slab(fr, used, dev), {f: k for k, f in enumerate(used)}


def _is_whole(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and bool(np.isfinite(v))


def _box_iou(a, b):
    """IoU of two (top, right, bottom, left) boxes: integer areas, the quotient in float64."""
    ih = min(a[2], b[2]) - max(a[0], b[0])
    iw = min(a[1], b[1]) - max(a[3], b[3])
    inter = ih * iw if ih > 0 and iw > 0 else 0
    union = (a[2] - a[0]) * (a[1] - a[3]) + (b[2] - b[0]) * (b[1] - b[3]) - inter
    return float(inter) / float(union) if union > 0 else 0.0


def track_boxes(boxes, iou=0.3, max_gap=1, return_anchors=False, cuts=None):
    """Link face boxes into tracks.  ``boxes``: rows (frame, top, right, bottom, left) in any order; they are taken frame by
    frame, ascending.  In frame f a live track (last seen in [f - max_gap, f)) and a box are a candidate pair when the IoU
    of the box with the track's last box is at least ``iou``; pairs are taken greedily by descending IoU (ties: lower track
    id, then earlier box row), one box per track and one track per box.  A box left over opens a new track; tracks are
    numbered by first appearance.  Frames a track skipped (max_gap > 1: a detector run on every k-th frame) are filled by
    per-coordinate linear interpolation between the two boxes around the gap, floor(a + (b - a) t + 0.5): each coordinate
    stays between its two ends, and top < bottom, left < right carry over because x -> floor(x + 0.5) is monotone and
    the ends differ by at least one — so the filled boxes lie inside the frame whenever both ends do and need no clipping.
    Returns a list of tracks, each a list of (frame, top, right, bottom, left) over consecutive frames; with
    ``return_anchors=True`` the pair (tracks, anchors), ``anchors[t][i]`` telling whether box i of track t was detected
    (an input row) rather than filled.
    ``cuts``: frame numbers at which a new shot starts (``shot_cuts``).  A track whose last box is in frame l is live for
    frame f only if no cut c has l < c <= f: a track never crosses a cut, and since only the gaps inside a track are
    filled, no box is interpolated across one.  ``None`` and an empty list change nothing."""
    rows = [tuple(int(v) for v in b) for b in boxes]
    cuts = [int(c) for c in cuts] if cuts is not None else []
    by_frame = {}
    for i, b in enumerate(rows):
        by_frame.setdefault(b[0], []).append(i)
    tracks = []                                             # per track: the boxes seen, ascending frames
    for f in sorted(by_frame):
        live = [t for t, tr in enumerate(tracks) if f - max_gap <= tr[-1][0] < f and
                not any(tr[-1][0] < c <= f for c in cuts)]
        pairs = []
        for t in live:
            for i in by_frame[f]:
                v = _box_iou(tracks[t][-1][1:], rows[i][1:])
                if v >= iou:
                    pairs.append((-v, t, i))
        used_t, used_i = set(), set()
        for _, t, i in sorted(pairs):
            if t not in used_t and i not in used_i:
                used_t.add(t)
                used_i.add(i)
                tracks[t].append(rows[i])
        for i in by_frame[f]:
            if i not in used_i:
                tracks.append([rows[i]])
    out = []
    for tr in tracks:
        full = [tr[0]]
        for a, b in zip(tr, tr[1:]):
            g = b[0] - a[0]
            for k in range(1, g):
                full.append((a[0] + k,) + tuple(int(np.floor(a[c] + (b[c] - a[c]) * (k / g) + 0.5)) for c in range(1, 5)))
            full.append(b)
        out.append(full)
    if return_anchors:
        seen = [{b[0] for b in tr} for tr in tracks]
        return out, [[b[0] in s for b in full] for full, s in zip(out, seen)]
    return out


def _check_follow(what, grid, radius):
    if grid not in _lib.TRACK_GRIDS or not 0 <= radius <= _lib.TRACK_RADIUS_MAX:
        raise ValueError(f"{what}: grid {grid} must be 16, 32 or 64 and radius {radius} lie in 0 ... {_lib.TRACK_RADIUS_MAX}")


def follow_tracks(frames, tracks, anchors, grid=64, radius=16, max_frames=128, dev=None):
    """Move the filled boxes of ``tracks`` onto the face: ``track_boxes`` fills the frames a detector skipped by linear
    interpolation, which a head that turns, nods or moves on a curve inside the gap leaves behind.  Every filled box
    between two detected boxes of its track (``anchors``, as ``track_boxes(..., return_anchors=True)`` returns them) is one
    job of ``_lib.track_match``: the interpolated box is the prior, the detections before and after the gap are the
    templates, and for frame fa + k of a gap g = fb - fa they weigh g - k and k, so the nearer one counts more.  The box
    moves by the (oy, ox) found, at most ``radius`` cells of its ``grid`` x ``grid`` lattice either way and never out of the
    frame; its size stays the interpolated one.  A filled box gets no job and stays as interpolated when one of the three
    boxes is lower or narrower than ``grid`` pixels, when g > 1024, and before the first or after the last detection.
    ``frames``: uint8 (F,H,W,3) RGB, numpy or a tensor.  Frames on the GPU are used in place, all jobs in one launch.  Of
    host frames the jobs go in (fa, fb, fs) order in groups launched one after another, a group being a run of jobs that
    needs at most ``max_frames`` (>= 3) distinct frames: only those are uploaded (to ``dev``, by default this module's
    ``device``), so device memory is bounded by the group, not the video.
    Returns ``(tracks, follow)``: the tracks with the filled boxes moved, and an int32 (n_jobs, 6) array of (track, frame,
    oy, ox, cost, cost0) rows in (track, frame) order — cost0 is the cost at the interpolated position.
    What this does not do: sub-cell refinement, a change of box size beyond the interpolation.  Extending a track past its
    first and last detection is ``extend_tracks``'s."""
    _check_follow("follow_tracks", grid, radius)
    if max_frames < 3:
        raise ValueError(f"follow_tracks: max_frames {max_frames} must be at least 3 (a job reads three frames)")
    fr = _as_frames("follow_tracks", frames)
    big = lambda b: b[3] - b[1] >= grid and b[2] - b[4] >= grid
    jobs = []                                               # (track, index in the track, the 17 integers)
    for t, (tr, flags) in enumerate(zip(tracks, anchors)):
        if len(tr) != len(flags):
            raise ValueError(f"follow_tracks: track {t} has {len(tr)} boxes and {len(flags)} anchor flags")
        seen = [i for i, d in enumerate(flags) if d]
        for ia, ib in zip(seen, seen[1:]):
            a, b = tr[ia], tr[ib]
            g = b[0] - a[0]
            if g > _lib.TRACK_WEIGHT_MAX or not (big(a) and big(b)):
                continue
            for i in range(ia + 1, ib):
                k = tr[i][0] - a[0]
                if 0 < k < g and big(tr[i]):
                    jobs.append((t, i, tuple(int(v) for v in (*tr[i], *a, g - k, *b, k))))
    out = [list(tr) for tr in tracks]
    follow = np.zeros((len(jobs), 6), dtype=np.int32)
    if not jobs:
        return out, follow
    res = np.zeros((len(jobs), 4), dtype=np.int64)
    if _resident(fr):
        res[:] = _lib.track_match(fr, [j[2] for j in jobs], grid=grid, radius=radius).cpu().numpy()
    else:
        groups, used = [], set()
        for n in sorted(range(len(jobs)), key=lambda n: (jobs[n][2][5], jobs[n][2][11], jobs[n][2][0], n)):
            need = {jobs[n][2][0], jobs[n][2][5], jobs[n][2][11]}
            if not groups or len(used | need) > max_frames:
                groups.append([])
                used = set()
            groups[-1].append(n)
            used |= need
        for ids in groups:
            slab, at = _upload(fr, sorted({jobs[n][2][c] for n in ids for c in (0, 5, 11)}), dev or device)
            rows = [tuple(at[v] if c in (0, 5, 11) else v for c, v in enumerate(jobs[n][2])) for n in ids]
            res[ids] = _lib.track_match(slab, rows, grid=grid, radius=radius).cpu().numpy()
    for n, (t, i, row) in enumerate(jobs):
        f, top, right, bottom, left = out[t][i]
        oy, ox = int(res[n, 0]), int(res[n, 1])
        out[t][i] = (f, top + oy, right + ox, bottom + oy, left + ox)
        follow[n] = (t, f, oy, ox, res[n, 2], res[n, 3])
    return out, follow


EXTEND_DEFAULTS = dict(grid=64, radius=8, steps=16, cost_max=18.7)


def _check_extend(what, grid=EXTEND_DEFAULTS["grid"], radius=EXTEND_DEFAULTS["radius"], steps=EXTEND_DEFAULTS["steps"],
                  cost_max=EXTEND_DEFAULTS["cost_max"]):
    if not (_is_whole(grid) and grid in _lib.TRACK_GRIDS and _is_whole(radius) and 0 <= radius <= _lib.TRACK_RADIUS_MAX):
        raise ValueError(f"{what}: grid {grid} must be 16, 32 or 64 and radius {radius} lie in 0 ... {_lib.TRACK_RADIUS_MAX}")
    if not (_is_whole(steps) and 1 <= steps <= _lib.TRACK_CHAIN_STEPS_MAX):
        raise ValueError(f"{what}: steps {steps} must be an integer in 1 ... {_lib.TRACK_CHAIN_STEPS_MAX}")
    if not (_is_number(cost_max) and 0 <= cost_max <= 255):
        raise ValueError(f"{what}: cost_max {cost_max} must be a number in 0 ... 255 (grey levels per cell)")


def extend_tracks(frames, tracks, ends=None, grid=EXTEND_DEFAULTS["grid"], radius=EXTEND_DEFAULTS["radius"],
                  steps=EXTEND_DEFAULTS["steps"], cost_max=EXTEND_DEFAULTS["cost_max"], iou=0.3, max_frames=128, dev=None):
    """Carry ``tracks`` past their first and last box.  A track starts at its first detection and ends at its last; with a
    detector that runs on every k-th frame up to k - 1 frames at each end of every shot are never scored, and a detector
    drop-out longer than the tracker's gap (a head turned to profile) ends a track although the face is still there.
    Every track gets one forward chain from its last box and one backward chain from its first box (both are
    detections when the tracks come from ``track_boxes``): ``_lib.track_chain`` searches frame after frame for the cells
    of that box, each step around the box the step before found, at most ``radius`` cells of the ``grid`` x ``grid``
    lattice either way, with the box's size unchanged and the template not updated.
    A forward chain from a box in frame f covers the frames f + 1, f + 2, ...: at most ``steps`` of them, none past the last
    frame of the video and none at or past the smallest entry of ``ends`` above f.  A backward chain covers f - 1, f - 2,
    ...: at most ``steps``, none below 0 and none below the largest entry of ``ends`` that is <= f — it may include the
    first frame of its shot.  ``ends``: the frame numbers at which a new shot starts (what ``scan_frames`` hands to
    ``track_boxes``: the cuts and the borders of the transitions).  A track whose end box is lower or narrower than ``grid``
    pixels gets no chain.  A chain ends at the first step whose best cost exceeds floor(``cost_max`` grid^2): ``cost_max``
    is the mean absolute difference per cell, in grey levels.
    The accepted steps are then cut where they run into another track: first the forward chains in track order, then the
    backward chains in track order, and a chain ends before the first frame in which another track — its own boxes and
    the extensions accepted so far — has a box with IoU >= ``iou`` against the chain's box.  Where a detector drop-out split
    one face into two tracks, this keeps the face from being scored twice; the two tracks are not joined here
    (``scan_frames(persons=True)`` can link them).
    ``frames``: uint8 (F,H,W,3) RGB, numpy or a tensor.  Frames on the GPU are used in place, all chains in one launch.  Of
    host frames the chains go in groups launched one after another, a group needing at most ``max_frames`` (>= 2) distinct
    frames: only those are uploaded (to ``dev``, by default this module's ``device``).  A chain that does not fit is
    continued in the next group from the sum of its offsets so far, which gives the same boxes as one launch.
    Returns ``(tracks, extend)``: the tracks with the accepted boxes added in front and behind, still over consecutive
    frames, and an int32 (n, 7) array of (track, frame, dir, oy, ox, cost, cost0) rows, one per accepted step — the forward
    chains in track order, then the backward ones, each along its chain; (oy, ox) is the step from the chain's box in
    the frame before (dir = 1) or after (dir = -1), cost0 the cost of not moving.
    The default ``cost_max`` is a starting value from synthetic material (tests/extendutil.py: smooth random colour patterns
    of tests/personutil.py's kind, 64 ... 120 pixels a side, moving up to 3 cells a frame over a drifting smooth background
    under pixel noise of sigma 3, at grids 16, 32 and 64, the pattern removed part-way): there the largest cost per cell of
    a step that still follows the pattern is 9.8 and the smallest of a step after it is gone 27.6, and 18.7 lies midway.
    No accuracy on real faces is claimed — ``extend`` holds every cost: look at them and choose.
    What this does not do: a change of box size along a chain, sub-cell refinement, template update, joining the tracks a
    chain runs into."""
    _check_extend("extend_tracks", grid, radius, steps, cost_max)
    if max_frames < 2:
        raise ValueError(f"extend_tracks: max_frames {max_frames} must be at least 2 (a chain reads its template's frame and a "
                         f"frame to search)")
    fr = _as_frames("extend_tracks", frames)
    nf = int(fr.shape[0])
    ends = sorted({int(e) for e in ends}) if ends is not None else []
    out = [[tuple(int(v) for v in b) for b in tr] for tr in tracks]
    _lib._check_boxes("extend_tracks", [tr[k] for tr in out if tr for k in (0, -1)], *fr.shape[:3])
    stop = int(np.floor(float(cost_max) * grid * grid))
    chains = []                                             # (track, dir, the template box, number of steps)
    for d in (1, -1):
        for t, tr in enumerate(out):
            if not tr:
                continue
            b = tr[-1] if d == 1 else tr[0]
            if b[3] - b[1] < grid or b[2] - b[4] < grid:
                continue
            if d == 1:
                room = min([e for e in ends if e > b[0]] + [nf]) - 1 - b[0]
            else:
                room = b[0] - max([e for e in ends if e <= b[0]] + [0])
            if min(room, steps) >= 1:
                chains.append((t, d, b, min(room, steps)))
    found = [[] for _ in chains]                            # per chain: the (oy, ox, cost, cost0) of its steps up to the stop

    def row(c, k0, n, at=None):
        """the 11 integers of the steps k0 ... k0 + n - 1 of chain c; ``at`` maps frame numbers to a slab's (consecutive
        frames stay consecutive: the slab is sorted)"""
        _, d, b, _ = chains[c]
        fa, fs = b[0], b[0] + d * (k0 + 1)
        if at is not None:
            fa, fs = at[fa], at[fs]
        return (fa, *b[1:], fs, d, n, sum(s[0] for s in found[c]), sum(s[1] for s in found[c]), stop)

    def take(ids, got):
        """the rows of one launch: chain ids[i] = (c, k0, n) continues with got[i, :n] up to its first refusal row"""
        for (c, k0, n), rows in zip(ids, got):
            for r in rows[:n].tolist():
                if tuple(r) == _lib.TRACK_CHAIN_NONE:
                    break
                found[c].append(tuple(r))
    if chains and _resident(fr):
        ids = [(c, 0, ch[3]) for c, ch in enumerate(chains)]
        take(ids, _lib.track_chain(fr, [row(*i) for i in ids], grid=grid, radius=radius).cpu().numpy())
    elif chains:
        # groups of (chain, first step, steps) segments: a chain takes as many steps as still fit into the group's frames
        groups, used = [[]], set()
        for c in sorted(range(len(chains)), key=lambda c: (min(chains[c][2][0], chains[c][2][0] + chains[c][1]), c)):
            _, d, b, total = chains[c]
            k0 = 0
            while k0 < total:
                n, need = 0, {b[0]}
                while k0 + n < total and len(used | need | {b[0] + d * (k0 + n + 1)}) <= max_frames:
                    need.add(b[0] + d * (k0 + n + 1))
                    n += 1
                if n:
                    groups[-1].append((c, k0, n))
                    used |= need
                    k0 += n
                if k0 < total:
                    groups.append([])
                    used = set()
        for ids in groups:
            ids = [(c, k0, n) for c, k0, n in ids if len(found[c]) == k0]          # a chain that stopped is not continued
            if not ids:
                continue
            used = sorted({f for c, k0, n in ids for f in [chains[c][2][0]] + [chains[c][2][0] + chains[c][1] * (k + 1)
                                                                               for k in range(k0, k0 + n)]})
            slab, at = _upload(fr, used, dev or device)
            take(ids, _lib.track_chain(slab, [row(*i, at) for i in ids], grid=grid, radius=radius).cpu().numpy())
    # the collision rule, in the chains' order: forward in track order, then backward in track order
    at_frame = {}
    for t, tr in enumerate(out):
        for b in tr:
            at_frame.setdefault(b[0], []).append((t, b[1:]))
    rows = []
    for (t, d, b, _), steps_found in zip(chains, found):
        box, added = b, []
        for oy, ox, cost, cost0 in steps_found:
            box = (box[0] + d, box[1] + oy, box[2] + ox, box[3] + oy, box[4] + ox)
            if any(o != t and _box_iou(box[1:], ob) >= iou for o, ob in at_frame.get(box[0], ())):
                break
            at_frame.setdefault(box[0], []).append((t, box[1:]))
            added.append(box)
            rows.append((t, box[0], d, oy, ox, cost, cost0))
        out[t] = out[t] + added if d == 1 else added[::-1] + out[t]
    return out, np.asarray(rows, dtype=np.int32).reshape(-1, 7)


def _check_cuts(what, threshold, regions):
    if not 0.0 < threshold <= 1.0:
        raise ValueError(f"{what}: threshold {threshold} must lie in (0, 1]")
    if isinstance(regions, bool) or not isinstance(regions, int) or regions not in _lib.CUT_REGIONS:
        raise ValueError(f"{what}: regions {regions} must be 1, 2, 4 or 8")


def shot_cuts(frames, threshold=0.4, regions=4, max_frames=128, dev=None):
    """Where the hard cuts of a video are.  ``track_boxes`` links faces by position alone, and after a cut the face of
    another person often sits where the last one sat; a track must end there.  Every frame is cut into ``regions`` x
    ``regions`` parts (R = 1, 2, 4 or 8; part (u, v) covers rows [(u H) // R, ((u + 1) H) // R) and the columns alike), each
    part gets a 64-bin luma histogram (``_lib.frame_hist``), and ``_lib.hist_diff`` gives dist[p][r], the L1 distance
    between the histograms of part r in frames p and p + 1 — integers, at most twice the part's pixel count n_r.  The score
    of the pair p keeps the max(1, R^2 // 2) parts with the smallest (dist[p][r], r):
        scores[p] = sum of the kept dist / (2 * sum of the kept n_r),   a value in [0, 1].
    Dropping the half of the parts that changed most keeps a moving head from counting as a cut; a cut changes every part.
    ``frames``: uint8 (F,H,W,3) RGB, numpy or a tensor.  Frames on the GPU are used in place: one ``frame_hist`` and one
    ``hist_diff`` launch.  Host frames are uploaded (to ``dev``, by default this module's ``device``) in consecutive groups of
    at most ``max_frames``, one ``frame_hist`` launch per group into its rows of a single (F, R^2, 64) device buffer (4 KB
    a frame at R = 4), then one ``hist_diff`` over the whole buffer: device memory for pixels is bounded by the group, not
    the video.
    Returns ``(cuts, scores)``: ``scores`` float64 numpy (F - 1,), and ``cuts`` the ascending frame numbers c = p + 1 with
    scores[p] >= ``threshold`` — a new shot starts at frame c.  F <= 1 gives ([], empty) and launches nothing; a
    ``threshold`` outside (0, 1] is a ValueError.
    What this does not do: only hard cuts are found here — linear fades and dissolves are ``shot_transitions``'s to find,
    eased ones and wipes nobody's; a one-frame flash gives two adjacent
    cuts; two shots with the same luma distribution in every part are not separated.  The default threshold is a starting
    value from synthetic material (about 0.05 inside a shot, about 0.7 at a cut); no accuracy is claimed — look at the
    scores and choose."""
    _check_cuts("shot_cuts", threshold, regions)
    if max_frames < 1:
        raise ValueError(f"shot_cuts: max_frames {max_frames} must be at least 1")
    fr = _as_frames("shot_cuts", frames)
    nf, h, w = (int(v) for v in fr.shape[:3])
    if nf <= 1:
        return [], np.empty((0,), dtype=np.float64)
    return _cuts_of(_frame_stats(fr, regions, None, max_frames, dev)[0], h, w, regions, threshold)


def _frame_stats(fr, regions, grid, max_frames, dev):
    """One pass over the frames (F >= 1) for ``shot_cuts`` and ``shot_transitions``: ``(hist, cells)``, the (F, R^2, 64)
    histograms of ``_lib.frame_hist`` and the (F, G^2) cell sums of ``_lib.frame_cells``; ``regions`` or ``grid`` None leaves
    that one out.  Device frames are used in place; host frames are uploaded once each, in consecutive groups of at most
    ``max_frames``, and every group fills its rows of the two device buffers."""
    if _resident(fr):
        return (_lib.frame_hist(fr, regions) if regions else None), (_lib.frame_cells(fr, grid) if grid else None)
    nf, d = int(fr.shape[0]), dev or device
    hist = torch.empty((nf, regions * regions, _lib.CUT_BINS), dtype=torch.int32, device=d) if regions else None
    cells = torch.empty((nf, grid * grid), dtype=torch.int32, device=d) if grid else None
    for g in range(0, nf, max_frames):
        slab = _rgb_slab(fr, slice(g, g + max_frames), d)
        if regions:
            _lib.frame_hist(slab, regions, out=hist[g:g + max_frames])
        if grid:
            _lib.frame_cells(slab, grid, out=cells[g:g + max_frames])
    return hist, cells


def _hist_scores(dist, h, w, regions):
    """The score of every row of a ``hist_diff`` / ``hist_diff_lag`` result, as ``shot_cuts`` defines it: float64 (rows,)."""
    dist = dist.cpu().numpy().view(np.uint32).astype(np.int64)                                # (rows, R^2)
    ey = [(u * h) // regions for u in range(regions + 1)]
    ex = [(v * w) // regions for v in range(regions + 1)]
    pixels = np.array([(ey[u + 1] - ey[u]) * (ex[v + 1] - ex[v]) for u in range(regions) for v in range(regions)],
                      dtype=np.int64)
    kept = np.argsort(dist, axis=1, kind="stable")[:, :max(1, regions * regions // 2)]       # ties: the lower r
    return np.take_along_axis(dist, kept, 1).sum(1) / (2.0 * pixels[kept].sum(1))


def _cuts_of(hist, h, w, regions, threshold):
    """``shot_cuts``'s result from the histograms of F >= 2 frames"""
    scores = _hist_scores(_lib.hist_diff(hist), h, w, regions)
    return [int(p) + 1 for p in np.nonzero(scores >= threshold)[0]], scores


TRANSITION_DEFAULTS = dict(lags=(4, 8), grid=16, h_min=0.25, rho_max=0.05, a_lo=0.1, a_hi=0.9, slack=0.05)


def _check_transitions(what, regions, lags, grid, h_min, rho_max, a_lo, a_hi, slack):
    if not _is_whole(regions) or regions not in _lib.CUT_REGIONS:
        raise ValueError(f"{what}: regions {regions} must be 1, 2, 4 or 8")
    if not _is_whole(grid) or grid not in _lib.CELL_GRIDS:
        raise ValueError(f"{what}: grid {grid} must be 8, 16 or 32")
    if not (isinstance(lags, (list, tuple)) and len(lags) > 0 and all(_is_whole(v) and 3 <= v <= _lib.FIT_LAGS[1] for v in lags)
            and len(set(lags)) == len(lags)):
        raise ValueError(f"{what}: lags {lags} must be distinct integers in 3 ... {_lib.FIT_LAGS[1]} (a span needs two frames "
                         f"between its ends)")
    if not (all(_is_number(v) for v in (h_min, rho_max, a_lo, a_hi, slack)) and 0.0 <= h_min <= 1.0 and rho_max >= 0.0
            and 0.0 <= a_lo < a_hi <= 1.0 and slack >= 0.0):
        raise ValueError(f"{what}: h_min {h_min} must lie in [0, 1], rho_max {rho_max} and slack {slack} be at least 0 and "
                         f"0 <= a_lo {a_lo} < a_hi {a_hi} <= 1")


def _transitions_of(hist, cells, nf, h, w, regions, lags, h_min, rho_max, a_lo, a_hi, slack):
    """``shot_transitions``'s result from the histograms and the cells of the ``nf`` frames (both unused, and possibly None,
    when no lag is below ``nf``)."""
    marked, info = set(), {}
    for lag in (int(v) for v in lags):
        if nf > lag:
            fit = _lib.blend_fit(cells, lag).cpu().numpy()                                    # (F - L, 2 L - 1) int64
            scores = _hist_scores(_lib.hist_diff_lag(hist, lag), h, w, regions)
        else:
            fit, scores = np.zeros((0, 2 * lag - 1), dtype=np.int64), np.zeros((0,), dtype=np.float64)
        some = fit[:, 0] > 0
        sdd = np.where(some, fit[:, 0].astype(np.float64), 1.0)[:, None]
        smd, smm = fit[:, 1:lag].astype(np.float64), fit[:, lag:].astype(np.float64)          # floats before any product
        a = np.where(some[:, None], smd / sdd, 0.0)
        rho = np.where(some[:, None], (smm - smd * smd / sdd) / sdd, np.inf)
        inside = (a >= a_lo) & (a <= a_hi)
        blend = (some & (scores >= h_min) & (rho.max(1) <= rho_max) & (a[:, 1:] >= a[:, :-1] - slack).all(1) &
                 (inside.sum(1) >= 2))
        for p in np.nonzero(blend)[0]:
            marked |= {int(p) + 1 + int(k) for k in np.nonzero(inside[p])[0]}
        info[lag] = {"scores": scores, "a": a, "rho": rho, "blend": blend}
    out = []
    for f in sorted(marked):
        if out and out[-1][1] == f - 1:
            out[-1] = (out[-1][0], f)
        else:
            out.append((f, f))
    return out, info


def shot_transitions(frames, lags=(4, 8), grid=16, regions=4, h_min=0.25, rho_max=0.05, a_lo=0.1, a_hi=0.9, slack=0.05,
                     max_frames=128, dev=None):
    """Where the fades and dissolves of a video are.  A linear dissolve makes every frame between its ends a pixelwise
    blend (1 - a) A + a B of the two end pictures with a rising (a fade is a dissolve to or from a flat frame), so on a
    ``grid`` x ``grid`` lattice of luma sums (``_lib.frame_cells``, G = 8, 16 or 32) the cell vector of a middle frame lies on
    the straight line between the cell vectors of the ends; motion, cuts and flashes leave that line.  For every lag L of
    ``lags`` (integers in 3 ... 32) and every span p of frames p ... p + L, ``_lib.blend_fit`` gives the exact integer sums
    Sdd, Smd_k, Smm_k of D = cells[p + L] - cells[p] and M_k = cells[p + k] - cells[p], k = 1 ... L - 1, from which, in
    float64 (the integers are converted before anything is multiplied),
        a_k = Smd_k / Sdd               where frame p + k lies on the line, 0 at p and 1 at p + L
        rho_k = (Smm_k - Smd_k^2 / Sdd) / Sdd   its squared distance from the line over the line's squared length.
    Slow motion is linear in the cells to first order too, but keeps the luma distribution, which a blend does not: the
    ends of a span must also differ by the score of ``shot_cuts`` taken at the lag L (``_lib.frame_hist`` on ``regions`` x
    ``regions`` parts, ``_lib.hist_diff_lag``).  Span p is a blend span iff
        Sdd > 0,  that score >= ``h_min``,  max_k rho_k <= ``rho_max``,  a_(k+1) >= a_k - ``slack`` for all k,
        and at least two k have ``a_lo`` <= a_k <= ``a_hi``;
    those frames p + k of it are marked.  The union over all spans and lags is taken, and the maximal runs of marked frames
    are the transitions.
    ``frames``: uint8 (F,H,W,3) RGB, numpy or a tensor.  Frames on the GPU are used in place.  Host frames are uploaded (to
    ``dev``, by default this module's ``device``) once each, in consecutive groups of at most ``max_frames``, every group one
    ``frame_cells`` and one ``frame_hist`` launch into its rows of a single (F, G^2) and a single (F, R^2, 64) device buffer;
    the fits then run over the whole buffers, so device memory for pixels is bounded by the group, not the video.
    Returns ``(transitions, info)``: ``transitions`` the list of (first, last), frames inclusive and ascending, and
    ``info[L]`` for every lag a dict of ``scores`` (F - L,), ``a`` and ``rho`` (F - L, L - 1), all float64 (a = 0 and rho = inf
    where Sdd = 0), and ``blend`` (F - L,) bool: which spans passed — to look at and choose thresholds by.  A lag that is
    not below F gives empty arrays and launches nothing.  Bad ``lags``, ``grid``, ``regions`` or thresholds are a ValueError.
    What this does not do: non-linear (eased) dissolves, whose a_k still rise but whose frames this marks only as far as
    they stay near the line; wipes; transitions shorter than 3 frames (a span needs two frames strictly between its ends); a
    pan whose content change passes ``h_min`` is not told from a blend.  The defaults are starting values from synthetic
    material (there the accepted spans have rho <= 0.038 and scores >= 0.79, the spans of moving shots that pass every
    other test rho >= 0.058, and a pan of one pixel a frame scores <= 0.19); no accuracy is claimed — look at ``info`` and
    choose."""
    _check_transitions("shot_transitions", regions, lags, grid, h_min, rho_max, a_lo, a_hi, slack)
    if max_frames < 1:
        raise ValueError(f"shot_transitions: max_frames {max_frames} must be at least 1")
    fr = _as_frames("shot_transitions", frames)
    nf, h, w = (int(v) for v in fr.shape[:3])
    hist, cells = _frame_stats(fr, regions, grid, max_frames, dev) if nf > min(lags) else (None, None)
    return _transitions_of(hist, cells, nf, h, w, regions, lags, h_min, rho_max, a_lo, a_hi, slack)


QUALITY_DEFAULTS = dict(grid=64, sharp_rel=0.5, sharp_min=0.0, clip_max=0.5)


def _check_quality(what, grid=64, sharp_rel=0.5, sharp_min=0.0, clip_max=0.5):
    if not _is_whole(grid) or grid not in _lib.TRACK_GRIDS:
        raise ValueError(f"{what}: grid {grid} must be 16, 32 or 64")
    if not (all(_is_number(v) for v in (sharp_rel, sharp_min, clip_max)) and 0.0 <= sharp_rel <= 1.0 and sharp_min >= 0.0
            and 0.0 < clip_max <= 1.0):
        raise ValueError(f"{what}: sharp_rel {sharp_rel} must lie in [0, 1], sharp_min {sharp_min} be at least 0 and clip_max "
                         f"{clip_max} lie in (0, 1]")


def _box_groups(fr, rows, ids, max_frames, dev):
    """The boxes ``ids`` of ``rows`` in frame order, cut into runs that lie on at most ``max_frames`` distinct frames; per run
    (its ids, those frames of the host frames ``fr`` as a slab on ``dev``, its rows with the frame counted within the slab):
    what one upload serves."""
    groups, used = [], set()
    for i in sorted(ids, key=lambda i: (rows[i][0], i)):
        if not groups or len(used | {rows[i][0]}) > max_frames:
            groups.append([])
            used = set()
        groups[-1].append(i)
        used.add(rows[i][0])
    for group in groups:
        slab, at = _upload(fr, sorted({rows[i][0] for i in group}), dev)
        yield group, slab, [(at[rows[i][0]], *rows[i][1:]) for i in group]


def face_quality(frames, boxes, grid=64, max_frames=128, dev=None):
    """How usable is each face crop.  A face smeared by motion or defocus, blown out by a flash or lost in the dark still
    gets a crop and a score, and the score is noise at best.  Every box is measured on its own ``grid`` x ``grid`` lattice
    of mean-luma cells c[u][v] (``_lib.face_quality``, G = 16, 32 or 64; include/genconvit_hip.h states the integer
    arithmetic): L2, the sum of squares of the cells' discrete Laplacian over the interior, which blur removes first; GX
    and GY, the sums of squared differences along the rows and down the columns, whose ratio tells the direction of a
    motion blur; the sum and the sum of squares of the cells; and the numbers of cells below 16 and above 239.
    ``frames``: uint8 (F,H,W,3) RGB, numpy or a tensor.  Frames on the GPU are used in place, all boxes in one launch.  Of
    host frames the boxes go in frame order in groups launched one after another, a group being a run of boxes that lie
    on at most ``max_frames`` (>= 1) distinct frames: only those are uploaded (to ``dev``, by default this module's
    ``device``), so device memory is bounded by the group, not the video.  ``boxes``: rows (frame, top, right, bottom, left)
    inside their frames.  A box lower or narrower than ``grid`` pixels is not sent: it comes back unmeasured.
    Returns a dict of numpy arrays in the order of ``boxes``:
      raw          (n,8) int64 rows (G, S1, S2, L2, GX, GY, dark, bright); zeros where not measured
      measured     bool
      sharpness    L2 / (G - 2)^2, the mean squared Laplacian of an interior cell
      gx, gy       GX / (G (G - 1)) and GY / (G (G - 1)), the mean squared difference between neighbours in a row, in a column
      mean         S1 / G^2
      contrast     S2 / G^2 - mean^2, the variance of the cells
      dark, bright the fractions of the G^2 cells below 16 and above 239
    all float64 but the first two, and NaN where ``measured`` is false.  No box: empty arrays, nothing is launched.
    What the grid cannot see: blur finer than a cell (box side / G pixels) is invisible, so ``grid`` should follow the face
    size.  On the CPU restatement of the arithmetic, a 9-pixel box blur of a texture with 4-pixel features lowers L2 of
    a 200-pixel face about 30-fold at G = 64 (a cell is 3 pixels) and about 2-fold at G = 16 (a cell is 12:
    tests/test_quality_cpu.py).  Nothing here judges: the
    thresholds are ``quality_keep``'s, and the caller's to choose."""
    _check_quality("face_quality", grid=grid)
    if max_frames < 1:
        raise ValueError(f"face_quality: max_frames {max_frames} must be at least 1")
    fr = _as_frames("face_quality", frames)
    grid = int(grid)
    rows = [tuple(int(v) for v in b) for b in boxes]
    _lib._check_boxes("face_quality", rows, *fr.shape[:3])
    n = len(rows)
    raw = np.zeros((n, 8), dtype=np.int64)
    big = [i for i, b in enumerate(rows) if b[3] - b[1] >= grid and b[2] - b[4] >= grid]
    if big and _resident(fr):
        raw[big] = _lib.face_quality(fr, [rows[i] for i in big], grid=grid).cpu().numpy()
    elif big:
        for ids, slab, local in _box_groups(fr, rows, big, max_frames, dev or device):
            raw[ids] = _lib.face_quality(slab, local, grid=grid).cpu().numpy()
    measured = np.zeros(n, dtype=bool)
    measured[big] = True
    g = float(grid)
    value = lambda v: np.where(measured, v, np.nan)
    s1, s2, l2, gx, gy, dark, bright = (raw[:, k].astype(np.float64) for k in range(1, 8))
    mean = s1 / (g * g)
    return {"raw": raw, "measured": measured, "sharpness": value(l2 / ((g - 2) * (g - 2))),
            "gx": value(gx / (g * (g - 1))), "gy": value(gy / (g * (g - 1))), "mean": value(mean),
            "contrast": value(s2 / (g * g) - mean * mean), "dark": value(dark / (g * g)), "bright": value(bright / (g * g))}


def quality_keep(quality, track_offsets, sharp_rel=0.5, sharp_min=0.0, clip_max=0.5):
    """Which rows of ``face_quality``'s result are fit to be scored: a bool array, True = keep.  ``quality``: that dict, over
    the rows of all tracks concatenated; ``track_offsets``: track t owns the rows [track_offsets[t], track_offsets[t + 1]),
    from 0 to the number of rows.  A measured row is dropped when any of these holds:
      sharpness < ``sharp_rel`` x the median sharpness of the measured rows of its track (``numpy.median``: the mean of the
                  two middle values of an even count) — the track's own median cancels the person, the lighting and the
                  face size, which set the absolute level;
      sharpness < ``sharp_min``, an absolute floor (0 by default: off);
      dark > ``clip_max`` or bright > ``clip_max``: more than that fraction of the cells is below 16, or above 239.
    Unmeasured rows (a face smaller than the grid) are kept: nothing is known against them.  ``sharp_rel`` outside [0, 1], a
    negative ``sharp_min``, ``clip_max`` outside (0, 1] and offsets that do not cover the rows are a ValueError.
    The three defaults are starting values from synthetic material (a noise texture with 4-pixel features, box blurs of 9
    and 15 pixels, flat, black and white patches); no accuracy on real footage is claimed — the numbers are in ``quality``:
    look at them and choose."""
    _check_quality("quality_keep", sharp_rel=sharp_rel, sharp_min=sharp_min, clip_max=clip_max)
    measured = np.asarray(quality["measured"], dtype=bool)
    sharp, dark, bright = (np.asarray(quality[k], dtype=np.float64) for k in ("sharpness", "dark", "bright"))
    offs = [int(v) for v in track_offsets]
    n = len(measured)
    if not (len(offs) >= 1 and offs[0] == 0 and offs[-1] == n and all(a <= b for a, b in zip(offs, offs[1:]))):
        raise ValueError(f"quality_keep: track_offsets must rise from 0 to the {n} rows of quality")
    keep = np.ones(n, dtype=bool)
    for lo, hi in zip(offs, offs[1:]):
        m = measured[lo:hi]
        if not m.any():
            continue
        s = np.where(m, sharp[lo:hi], 0.0)
        bad = (s < sharp_rel * np.median(s[m])) | (s < sharp_min) | (np.where(m, dark[lo:hi], 0.0) > clip_max) | \
              (np.where(m, bright[lo:hi], 0.0) > clip_max)
        keep[lo:hi] = ~(m & bad)
    return keep


PERSON_DEFAULTS = dict(link_max=9082, per_track=64)


def _check_persons(what, link_max=PERSON_DEFAULTS["link_max"], per_track=PERSON_DEFAULTS["per_track"]):
    if not (_is_number(link_max) and link_max >= 0):
        raise ValueError(f"{what}: link_max {link_max} must be a number of at least 0")
    if not _is_whole(per_track) or per_track < 1:
        raise ValueError(f"{what}: per_track {per_track} must be an integer of at least 1")


def face_signatures(frames, boxes, max_frames=128, dev=None):
    """What each face crop looks like, for telling people apart: per box the 384 bytes of ``_lib.face_signature`` (the
    mean-luma cells of a 16 x 16 grid with the box's own mean and spread taken out, which cancels the gain and offset of a
    shot's exposure, then Cb and Cr on an 8 x 8 grid; include/genconvit_hip.h states the integer arithmetic).
    ``frames``: uint8 (F,H,W,3) RGB, numpy or a tensor.  Frames on the GPU are used in place, all boxes in one launch.  Of
    host frames the boxes go in frame order in groups launched one after another, a group being a run of boxes that lie
    on at most ``max_frames`` (>= 1) distinct frames: only those are uploaded (to ``dev``, by default this module's
    ``device``), as in ``face_quality``.  ``boxes``: rows (frame, top, right, bottom, left) inside their frames.  A box lower
    or narrower than 16 pixels is not sent: it comes back unmeasured.  Returns a dict in the order of ``boxes``:
      sig        (n,384) uint8 on the device; zeros where not measured
      measured   bool (n,), numpy
    No box: empty arrays, nothing is launched.  The signature is a coarse picture of the box, not an identity embedding:
    two people in like clothes before one wall at one pose can come close, and one person in profile and en face does
    not."""
    if max_frames < 1:
        raise ValueError(f"face_signatures: max_frames {max_frames} must be at least 1")
    fr = _as_frames("face_signatures", frames)
    rows = [tuple(int(v) for v in b) for b in boxes]
    _lib._check_boxes("face_signatures", rows, *fr.shape[:3])
    n, g = len(rows), _lib.SIG_GRID
    to = fr.device if fr.is_cuda else (dev or device)
    big = [i for i, b in enumerate(rows) if b[3] - b[1] >= g and b[2] - b[4] >= g]
    measured = np.zeros(n, dtype=bool)
    measured[big] = True
    if not big:
        return {"sig": torch.empty((0, _lib.SIG_BYTES), dtype=torch.uint8, device=to) if n == 0 else
                torch.zeros((n, _lib.SIG_BYTES), dtype=torch.uint8, device=to), "measured": measured}
    if _resident(fr):
        parts, order = [_lib.face_signature(fr, [rows[i] for i in big])], list(big)
    else:
        parts, order = [], []
        for ids, slab, local in _box_groups(fr, rows, big, max_frames, to):
            parts.append(_lib.face_signature(slab, local))
            order += ids
    got = torch.cat(parts)
    if order == list(range(n)):
        return {"sig": got, "measured": measured}
    sig = torch.zeros((n, _lib.SIG_BYTES), dtype=torch.uint8, device=got.device)
    sig[torch.as_tensor(order, device=got.device)] = got
    return {"sig": sig, "measured": measured}


def link_tracks(dist, tracks, link_max=PERSON_DEFAULTS["link_max"]):
    """Which tracks are one person: ``persons``, a list of sorted lists of track numbers, ordered by each person's lowest
    track.  ``dist``: (T,T) integers, ``dist[a][b]`` the distance between the two most alike crops of the tracks a and b
    (``_lib.sig_link``; read above the diagonal); ``tracks``: the T tracks, lists of rows (frame, ...).  Single linkage with
    a veto: the pairs a < b with ``dist[a][b] <= link_max`` are taken in ascending (dist, a, b) order, and the clusters of
    a and b become one unless the two clusters have a frame number in common — two faces in one frame are two people,
    however alike, and so is everything already joined to either.  A pair that is vetoed stays apart even if a later
    pair lies close: clusters only grow, so what shares a frame once shares it for good.  ``0xFFFFFFFF``
    (no measured crop in one of the tracks) never links, whatever ``link_max``.  A ``dist`` that is not (T,T) and a
    negative ``link_max`` are a ValueError.
    The default ``link_max`` is a starting value from synthetic material (tests/personutil.py: smooth random colour
    patterns seen again under gain 0.8 ... 1.15, offset +-20, shifts of a few pixels, box sides 64 ... 200 and noise of
    sigma 3): there the largest distance between two shots of one pattern is 5 804 and the smallest between shots of two
    patterns 12 361, and 9 082 is the integer midway.  No accuracy on real faces is claimed — ``scan_frames`` returns the
    matrix: look at it and choose."""
    _check_persons("link_tracks", link_max=link_max)
    T = len(tracks)
    d = np.asarray(dist.cpu() if torch.is_tensor(dist) else dist, dtype=np.int64).reshape(-1)
    if d.size != T * T:
        raise ValueError(f"link_tracks: dist holds {d.size} values for {T} tracks")
    d = d.reshape(T, T)
    pairs = sorted((int(d[a, b]), a, b) for a in range(T) for b in range(a + 1, T)
                   if d[a, b] <= link_max and d[a, b] != _lib.SIG_NONE)
    root = list(range(T))
    members = [[t] for t in range(T)]
    seen = [{int(r[0]) for r in tr} for tr in tracks]

    def find(t):
        while root[t] != t:
            t = root[t]
        return t
    for _, a, b in pairs:
        ra, rb = find(a), find(b)
        if ra == rb or seen[ra] & seen[rb]:
            continue
        lo, hi = min(ra, rb), max(ra, rb)
        root[hi] = lo
        members[lo] += members[hi]
        seen[lo] |= seen[hi]
    return [sorted(members[t]) for t in range(T) if root[t] == t]


def _verdict(m):
    """(y, y_val) of a mean pair, as ``max_prediction_value`` / ``pred_vids`` compute it."""
    return int(torch.argmax(m).item()), m[0].item() if m[0] > m[1] else abs(1 - m[1]).item()


def _scan_persons(fr, tracks, rows, offsets, logits, nets, max_batch, dev, link_max, per_track):
    """``scan_frames``'s ``persons`` (its docstring says what the keys hold); ``logits``: [net 0 all crops; net 1 all crops]
    in the order of ``rows``."""
    n, T = len(rows), len(tracks)
    sampled, owner = [], []
    for t, tr in enumerate(tracks):
        m = min(per_track, len(tr))
        sampled += [offsets[t] + (k * len(tr)) // m for k in range(m)]
        owner += [t] * m
    sigs = face_signatures(fr, [rows[i] for i in sampled], max_frames=max_batch, dev=dev)
    owner = [t if ok else -1 for t, ok in zip(owner, sigs["measured"].tolist())]
    distance = _lib.sig_link(sigs["sig"], owner, T).cpu().numpy().astype(np.int64)
    linked = link_tracks(distance, tracks, link_max)
    of_track = [0] * T
    perm, ranges = [], []
    for k, person in enumerate(linked):
        lo = len(perm)
        for t in person:
            of_track[t] = k
            perm += range(offsets[t], offsets[t + 1])
        ranges.append((lo, len(perm)))
    pick = torch.as_tensor([k * n + i for k in range(nets) for i in perm], device=logits.device)
    _, mean2 = _lib.vote_windows(logits.index_select(0, pick), n, nets, ranges)
    means = mean2.cpu()
    return {"tracks": linked, "of_track": of_track, "verdicts": [_verdict(means[k]) for k in range(len(linked))],
            "means": mean2, "distance": distance, "rows": sampled, "measured": sigs["measured"]}


_ScanOptions = collections.namedtuple("_ScanOptions", "follow cuts transitions targs extend eargs quality qargs persons pargs")


def _option_args(option, value, name, given, defaults, check, *lead, false_is_off=True):
    """One on/off option of ``scan_frames`` and its ``*_args``: ``defaults`` with the dict ``given`` laid over and checked
    (``check("scan_frames", *lead, **args)``) when the option is on, the defaults alone when it is off.  ``value`` must be
    None or True; False means off too, unless ``false_is_off`` is False."""
    if value is not None and value is not True and not (false_is_off and value is False):
        raise ValueError(f"scan_frames: {option} {value!r} must be None or True")
    args = dict(defaults)
    if value:
        if given is not None:
            if not (isinstance(given, dict) and set(given) <= set(args)):
                raise ValueError(f"scan_frames: {name} must be a dict with keys among {sorted(args)}")
            args.update(given)
        check("scan_frames", *lead, **args)
    return args


def _scan_options(nf, detect_every, window, stride, max_batch, follow, follow_grid, follow_radius, cuts, cut_threshold,
                  cut_regions, transitions, transition_args, quality, quality_args, persons, person_args, extend, extend_args):
    """The options stage of ``scan_frames``: every check that needs nothing but the arguments and the number of frames
    ``nf``, before the detector, ``track_boxes`` or any binding is reached.  Returns what the later stages read: which
    options are on, ``cuts`` and ``transitions`` as None, True or their sorted lists, and each ``*_args`` merged with its
    defaults."""
    eargs = _option_args("extend", extend, "extend_args", extend_args, EXTEND_DEFAULTS, _check_extend, false_is_off=False)
    qargs = _option_args("quality", quality, "quality_args", quality_args, QUALITY_DEFAULTS, _check_quality)
    pargs = _option_args("persons", persons, "person_args", person_args, PERSON_DEFAULTS, _check_persons)
    targs = _option_args("transitions", transitions is True or None, "transition_args", transition_args, TRANSITION_DEFAULTS,
                         _check_transitions, cut_regions)
    if transitions is not True and transitions is not None:
        given = list(transitions) if isinstance(transitions, (list, tuple)) else None
        if given is None or not all(isinstance(t, (list, tuple)) and len(t) == 2 and _is_whole(t[0]) and _is_whole(t[1]) and
                                    0 <= t[0] <= t[1] < nf for t in given):
            raise ValueError(f"scan_frames: transitions must be True or a list of (first, last) integer pairs with "
                             f"0 <= first <= last <= {nf - 1}")
        transitions = sorted({(int(t[0]), int(t[1])) for t in given})
    if cuts is True:
        _check_cuts("scan_frames", cut_threshold, cut_regions)
    elif cuts is not None:
        given = list(cuts) if isinstance(cuts, (list, tuple, np.ndarray)) else None
        if given is None or not all(_is_whole(c) and 1 <= c < nf for c in given):
            raise ValueError(f"scan_frames: cuts must be True or a list of integers in [1, {nf - 1}]")
        cuts = sorted({int(c) for c in given})
    if detect_every < 1 or max_batch < 1:
        raise ValueError(f"scan_frames: detect_every {detect_every} and max_batch {max_batch} must both be at least 1")
    window_ranges(1, window, stride)                        # bad window / stride: raise before anything runs
    if follow:
        _check_follow("scan_frames", follow_grid, follow_radius)
    return _ScanOptions(bool(follow), cuts, transitions, targs, bool(extend), eargs, bool(quality), qargs, bool(persons), pargs)


def _scan_shots(fr, opt, cut_threshold, cut_regions, max_batch, dev):
    """The shots stage of ``scan_frames``: the cuts and transitions that were asked for and not given, from one shared
    ``_frame_stats`` upload when both are computed.  Returns ``(cuts, cut_scores, transitions, transition_info, ends)``:
    the scores and the info are None where nothing was computed, and ``ends`` are the frames at which a new shot starts
    for ``track_boxes`` and ``extend_tracks`` — the cuts and the borders of the transitions."""
    cuts, transitions = opt.cuts, opt.transitions
    nf, h, w = (int(v) for v in fr.shape[:3])
    cut_scores = transition_info = None
    if transitions is True:
        targs = dict(opt.targs)
        lags, grid = targs.pop("lags"), targs.pop("grid")
        hist, cells = (_frame_stats(fr, cut_regions, grid, max_batch, dev)                        # one upload feeds both
                       if nf > (1 if cuts is True else min(lags)) else (None, None))
        transitions, transition_info = _transitions_of(hist, cells, nf, h, w, cut_regions, lags, **targs)
        if cuts is True:
            cuts, cut_scores = _cuts_of(hist, h, w, cut_regions, cut_threshold) if nf > 1 else ([], np.empty((0,), np.float64))
    elif cuts is True:
        cuts, cut_scores = shot_cuts(fr, cut_threshold, cut_regions, max_frames=max_batch, dev=dev)
    ends = cuts
    if transitions is not None:
        ends = sorted(set(cuts or []) | {c for first, last in transitions for c in (first, last + 1) if 1 <= c < nf})
    return cuts, cut_scores, transitions, transition_info, ends


def _scan_tracks(fr, boxes, transitions, ends, opt, detect_every, iou, follow_grid, follow_radius, max_batch, dev):
    """The tracks stage of ``scan_frames``: the boxes outside the transitions linked into tracks, then followed, extended
    and gated by quality as ``opt`` says.  Returns ``(tracks, follow, extend, quality)``, the last three as the result
    holds them, None for a step that is off."""
    moved = extended = measures = None
    if transitions is not None:
        boxes = [b for b in boxes if not any(first <= b[0] <= last for first, last in transitions)]
    if opt.follow:
        tracks, anchors = track_boxes(boxes, iou=iou, max_gap=detect_every, return_anchors=True, cuts=ends)
        tracks, moved = follow_tracks(fr, tracks, anchors, grid=follow_grid, radius=follow_radius,
                                      max_frames=max(max_batch, 3), dev=dev)
    else:
        tracks = track_boxes(boxes, iou=iou, max_gap=detect_every, cuts=ends)
    if opt.extend:
        tracks, extended = extend_tracks(fr, tracks, ends, iou=iou, max_frames=max(max_batch, 2), dev=dev, **opt.eargs)
    if opt.quality:
        qargs = dict(opt.qargs)
        before = [b for tr in tracks for b in tr]
        measures = face_quality(fr, before, grid=qargs.pop("grid"), max_frames=max_batch, dev=dev)
        kept = quality_keep(measures, np.cumsum([0] + [len(tr) for tr in tracks]), **qargs)
        left = iter(kept.tolist())
        tracks = [[b for b in tr if next(left)] for tr in tracks]
        measures.update(kept=kept, boxes=before, track_map=[t for t, tr in enumerate(tracks) if tr])
        tracks = [tr for tr in tracks if tr]
    return tracks, moved, extended, measures


def _scan_logits(fr, model, rows, eps, max_batch):
    """The crops stage of ``scan_frames``: the crop ``rows`` in frame order in groups of at most ``max_batch``, each one upload
    of the frames it lies on, one ``_lib.face_crop_preprocess`` and one model call.  Returns ``(logits, nets)``: the groups'
    [net 0 | net 1] logits put into [net 0 all crops; net 1 all crops] in the order of ``rows``."""
    p = next(model.parameters())
    n = len(rows)
    nets = 2 if getattr(model, "net", "genconvit") not in ("ed", "vae") else 1
    order = sorted(range(n), key=lambda i: (rows[i][0], i))             # frame order
    parts, src = [], [0] * (nets * n)
    for g in range(0, n, max_batch):
        ids = order[g:g + max_batch]
        slab, at = _upload(fr, sorted({rows[i][0] for i in ids}), p.device)     # the frames this group's crops lie on, no others
        x = _lib.face_crop_preprocess(slab, [(at[rows[i][0]], *rows[i][1:]) for i in ids], dtype=p.dtype)
        if eps is not None:
            logits = model(x, eps=eps[torch.as_tensor(ids, device=eps.device)].to(p.device))
        else:
            logits = model(x)
        if getattr(model, "reference_logits_dtype", False):
            logits = logits.to(p.dtype)
        parts.append(logits.reshape(-1, 2))
        for k in range(nets):                                           # this group's rows are [net 0 | net 1]
            for j, i in enumerate(ids):
                src[k * n + i] = nets * g + k * len(ids) + j
    return torch.cat(parts).index_select(0, torch.as_tensor(src, device=p.device)), nets


def _scan_votes(tracks, offsets, logits, nets, window, stride):
    """The votes stage of ``scan_frames``: ONE ``_lib.vote_windows`` call over every window of every track, every whole track
    and everything.  Returns the result's ``frame_scores``, ``window_means``, ``windows``, ``track_verdicts``, ``verdict`` and
    ``segments``."""
    n = offsets[-1]
    ranges, wins = [], []
    for t, tr in enumerate(tracks):
        for lo, hi in window_ranges(len(tr), window, stride):
            ranges.append((offsets[t] + lo, offsets[t] + hi))
            wins.append((t, tr[lo][0], tr[hi - 1][0]))
    ranges += [(offsets[t], offsets[t + 1]) for t in range(len(tracks))] + [(0, n)]
    frame_p, mean2 = _lib.vote_windows(logits, n, nets, ranges)
    means = mean2.cpu()
    nw = len(wins)
    windows = [(*w, *_verdict(means[k])) for k, w in enumerate(wins)]
    segments, run = [], None
    for t, first, last, y, y_val in windows + [(None, 0, 0, 1, 0.0)]:
        if run is not None and (y != 0 or t != run[0]):
            segments.append(tuple(run))
            run = None
        if y == 0:
            run = [t, first, last, y_val] if run is None else [t, run[1], last, max(run[3], y_val)]
    return {"frame_scores": frame_p, "window_means": mean2[:nw], "windows": windows,
            "track_verdicts": [_verdict(means[nw + t]) for t in range(len(tracks))],
            "verdict": _verdict(means[nw + len(tracks)]), "segments": segments}


def scan_frames(frames, model, boxes=None, locate=None, detect_every=1, iou=0.3, window=15, stride=1, max_batch=128,
                eps=None, follow=False, follow_grid=64, follow_radius=16, cuts=None, cut_threshold=0.4, cut_regions=4,
                transitions=None, transition_args=None, quality=None, quality_args=None, persons=None,
                person_args=None, extend=None, extend_args=None):
    """When is a video fake, and whose face: every face of every frame is scored, linked into per-person tracks, and voted
    over sliding windows of each track.  ``frames``: uint8 (F,H,W,3) RGB, numpy or a tensor on either device, or a ``YUV420``
    (decoder-native frames: every stage's groups are then uploaded as YUV, half the bytes, and converted on the device;
    the result is the one the same pixels give as host RGB frames.  With ``boxes=None`` the detector still wants RGB on
    the host: the frames ``[::detect_every]`` are converted on the device in groups of ``max_batch`` and downloaded, which
    is the price of a CPU detector — callers with their own boxes pay nothing).  ``boxes``:
    rows (frame, top, right, bottom, left); by default the detector — ``locate``, else ``face_locations(..., keep_all=True)``
    — runs on ``frames[::detect_every]``, handed over as a numpy array on the host whatever ``frames`` is, and its frame
    indices are mapped back.  ALL faces are kept: the ``len(frames)`` cut is ``face_rec``'s contract, not this function's,
    and the default detector is called without it.  Tracks: ``track_boxes(boxes, iou, max_gap=detect_every)``, which also fills the frames the detector
    skipped (``detect_every`` sets that gap for explicit ``boxes`` too).  The crops run in frame order in groups of at most
    ``max_batch``: of host frames only the frames a group's crops lie on are uploaded (at most ``max_batch`` of them, however
    far apart), so device memory is bounded by the group, not the video; each group is one ``_lib.face_crop_preprocess`` launch into the model's parameter dtype and one
    ``model(x)`` — ``model(x, eps=...)`` with the group's rows of ``eps`` (n_crops, latent), given in crop order.  The
    groups' [net 0 | net 1] logits are put into [net 0 all crops; net 1 all crops] in (track, frame) order on the device,
    and ONE ``_lib.vote_windows`` call votes every window of every track (``window_ranges(len, window, stride)``), every
    whole track and everything.  Returns a dict:
      tracks          the tracks, lists of (frame, top, right, bottom, left)
      boxes           the crop rows: the tracks concatenated, i.e. (track, frame) order — the order of everything below
      track_offsets   track t owns crop rows [track_offsets[t], track_offsets[t + 1])
      frame_scores    (n_crops, 2) fp32 on the device: per crop, the mean over the networks of sigmoid(logits)
      windows         [(track, first_frame, last_frame, y, y_val), ...], frames inclusive
      window_means    (n_windows, 2) fp32: the mean pair behind each window's (y, y_val)
      track_verdicts  [(y, y_val), ...]: ``pred_vid`` over each track's crops
      verdict         (y, y_val): ``pred_vid`` over all crops
      segments        [(track, first_frame, last_frame, peak y_val), ...]: the maximal runs of consecutive FAKE windows
                      (y == 0, what ``real_or_fake`` calls FAKE) of one track, from the first window's first frame to
                      the last window's last frame
    No face: ``verdict == (None, None)``, empty lists and tensors, and nothing is launched.  ``reference_logits_dtype`` is
    honoured as in ``pred_vid_explain``.
    ``follow=True`` (off by default; for ``detect_every`` > 1, without which no box is filled): before the crops are cut, the
    boxes that ``track_boxes`` filled are moved onto the face by block matching against the two detections around their gap
    (``follow_tracks`` with ``follow_grid``, ``follow_radius`` and ``max_batch`` as its ``max_frames``); ``tracks`` and
    ``boxes`` then hold the followed boxes and the result gains ``follow``, int32 (n_jobs, 6) rows (track, frame, oy, ox,
    cost, cost0).
    ``cuts`` (``None`` by default: nothing changes): the hard cuts of edited footage, at which every track ends — after a cut
    the face of another person often sits where the last one sat, and IoU alone would join the two.  ``True``:
    ``shot_cuts(frames, cut_threshold, cut_regions, max_frames=max_batch)`` over ALL scanned frames, not only the
    detector's (this runs even when no face is found); a list: the frame numbers at which a new shot starts, integers in
    [1, F - 1], anything else is a ValueError.  They go to ``track_boxes``, so no track, and therefore no window, no
    segment and no ``follow`` job, straddles a cut.  The result gains ``cuts``, and ``cut_scores`` (float64 (F - 1,)) when
    they were computed here: the default threshold is a starting value, not a tuned one.  With ``detect_every`` > 1 a face
    goes unscored between its last detection before a cut and its first detection after it unless ``extend`` carries the
    tracks there.  ``cuts`` finds hard cuts only, and a one-frame flash gives two adjacent cuts; linear fades and dissolves
    are what ``transitions`` is for.
    ``transitions`` (``None`` by default: nothing changes): the fades and dissolves of edited footage.  A dissolve from one
    talking head to another leaves a box where a box was, so IoU joins the two people, and the frames inside it show a
    blended face that is no evidence of anything.  ``True``: ``shot_transitions(frames, regions=cut_regions,
    max_frames=max_batch, **transition_args)`` over ALL scanned frames (``transition_args``: a dict of its ``lags``,
    ``grid``, ``h_min``, ``rho_max``, ``a_lo``, ``a_hi``, ``slack``; None: its defaults) — with ``cuts=True`` as well, every
    group of host frames is uploaded once and feeds both; a list: (first, last) pairs of integers, frames inclusive, 0 <=
    first <= last < F, anything else is a ValueError.  The boxes on the frames of a transition are dropped before tracking
    — they are not cut, scored or voted, and ``eps`` counts the crops that remain — and first and last + 1 join the cuts
    handed to ``track_boxes`` where they lie in [1, F - 1], so no track, window, segment or ``follow`` job reaches into or
    across a transition.  The result gains ``transitions`` (sorted), and ``transition_info`` (``shot_transitions``'s
    ``info``) when they were computed here; ``cuts`` keeps holding the hard cuts alone.  Linear blends of at least 3
    frames only: eased dissolves and wipes are not found, a fast pan can pass for one, and the thresholds are starting
    values, not tuned ones.
    ``quality`` (``None`` by default: nothing changes): faces that are themselves unusable — smeared by a head turn, out of
    focus, blown out by a flash, lost in the dark — get a crop, a score and a full vote like any other, and blur is what a
    blended face looks like.  ``True``: after tracking, and after ``follow`` so that the final boxes are the ones measured,
    ``face_quality(frames, rows, grid, max_frames=max_batch, dev=the model's device)`` measures every row and
    ``quality_keep`` says which stay (``quality_args``: a dict with keys among ``grid``, ``sharp_rel``, ``sharp_min``,
    ``clip_max``; None: their defaults; anything else is a ValueError, raised before anything runs).  The dropped rows
    leave their tracks before anything is cropped: they are not cut, scored or voted, and ``eps`` counts the crops that
    remain; a track that loses every row is removed, and a track that loses rows in its middle keeps one window over the
    hole.  ``tracks``, ``boxes``, ``track_offsets`` and everything after them describe the kept rows, and the result gains
    ``quality``: ``face_quality``'s dict over the rows before the gate, plus ``kept`` (bool per such row), ``boxes`` (those
    rows) and ``track_map`` (for each remaining track, its number before the gate).  The track column of ``follow`` counts
    the tracks before the gate.  With no face nothing is launched.  Host frames on which a measured box lies are uploaded
    a second time for this pass: the upload is not shared with the crops'.  The thresholds are starting values from
    synthetic material, not tuned ones, and blur finer than a cell of the grid is not seen.
    ``persons`` (``None`` by default: nothing changes): tracks end at every cut and transition, so an interview that cuts
    between two speakers comes back as dozens of short tracks, each with one weak vote, and nothing says which of them
    are one person.  ``True``: after tracking, ``follow`` and the ``quality`` gate, so that the final rows are the ones
    described, at most ``per_track`` rows of every track are sampled (row ``(k * len) // m`` for k < m = min(per_track,
    len)), ``face_signatures(frames, those rows, max_frames=max_batch, dev=the model's device)`` describes them, ONE
    ``_lib.sig_link`` gives the distance between the two most alike crops of every two tracks, ``link_tracks`` joins the
    tracks whose distance is at most ``link_max`` unless they share a frame, and a second ``_lib.vote_windows`` call votes
    over each person's rows (the logits ``index_select``-ed so that a person's rows are contiguous, in (track, frame)
    order).  ``person_args``: a dict with keys among ``link_max`` and ``per_track``; None: ``PERSON_DEFAULTS``; anything
    else is a ValueError, raised before anything runs.  The result gains ``persons``, a dict:
      tracks     the sorted track numbers of each person, ordered by each person's lowest track
      of_track   the person of each track
      verdicts   [(y, y_val), ...]: ``pred_vid`` over each person's crops (ALL rows of its tracks, not only the sampled)
      means      (P, 2) fp32 on the device: the mean pair behind each verdict
      distance   (T, T) int64 numpy: ``_lib.sig_link``'s matrix; 0xFFFFFFFF on the diagonal and for a track without a
                 measured row
      rows       the sampled crop rows, indices into ``boxes``
      measured   bool per sampled row: False for a box lower or narrower than 16 pixels, which takes no part
    With no face these are empty and nothing is launched.  Host frames on which a sampled row lies are uploaded once more
    for this pass: the upload is not shared with the crops'.  The default ``link_max`` (9 082) is a starting value from
    synthetic material — the largest distance between two shots of one pattern there is 5 804, the smallest between two
    patterns 12 361 (``link_tracks``) — not a tuned one: no accuracy on real faces is claimed, and ``distance`` is returned so
    that the caller can choose.
    ``extend`` (``None`` by default: nothing changes): a track starts at its first detection and ends at its last, so with
    ``detect_every`` = k up to k - 1 frames at each end of every shot are never scored, and a detector drop-out longer than
    k (a head turned to profile) ends a track for good.  ``True``: after ``track_boxes`` and ``follow``, and before the
    ``quality`` gate and ``persons`` so that both see the added rows, ``extend_tracks(frames, tracks, ends, iou=iou,
    max_frames=max_batch, dev=the model's device, **extend_args)`` carries every track backward from its first and forward
    from its last box by block matching (``_lib.track_chain``), with the ``ends`` that went to ``track_boxes``: no extension
    enters a transition or crosses a found cut.  ``extend_args``: a dict with keys among ``grid``, ``radius``, ``steps`` and
    ``cost_max``; None: ``EXTEND_DEFAULTS``; anything else is a ValueError, raised before anything runs.  ``tracks``,
    ``boxes`` and everything after them hold the extended tracks, ``eps`` counts the crops after extension, and the result
    gains ``extend``, int32 (n, 7) rows (track, frame, dir, oy, ox, cost, cost0), one per added box; the track column
    counts the tracks before the ``quality`` gate.  Without ``cuts`` only the cost gate stops a chain at a hard cut.
    Exposure drift raises the cost, so under it chains stop early: that is the safe side.  Where the detector did look at
    an extended frame, it is a frame on which it found nothing there.  The default ``cost_max`` is a starting value from
    synthetic material (``extend_tracks``), not a tuned one."""
    fr = _as_frames("scan_frames", frames)
    opt = _scan_options(int(fr.shape[0]), detect_every, window, stride, max_batch, follow, follow_grid, follow_radius, cuts,
                        cut_threshold, cut_regions, transitions, transition_args, quality, quality_args, persons, person_args,
                        extend, extend_args)
    if boxes is None:
        if isinstance(fr, YUV420):                          # the price of a CPU detector: see the docstring
            pick = list(range(0, len(fr), detect_every))
            dev = next(model.parameters()).device
            seen = torch.cat([fr.rgb(pick[g:g + max_batch], dev).cpu() for g in range(0, len(pick), max_batch)]).numpy() \
                if pick else np.empty((0, *fr.shape[1:]), dtype=np.uint8)
        else:
            seen = (fr.cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames))[::detect_every]
        found = locate(seen) if locate is not None else face_locations(seen, keep_all=True)
        boxes = [(int(b[0]) * detect_every, *b[1:]) for b in found]
    boxes = [tuple(int(v) for v in b) for b in boxes]
    _lib._check_boxes("scan_frames", boxes, *fr.shape[:3])
    p = next(model.parameters())
    cuts, cut_scores, transitions, transition_info, ends = _scan_shots(fr, opt, cut_threshold, cut_regions, max_batch, p.device)
    tracks, moved, extended, measures = _scan_tracks(fr, boxes, transitions, ends, opt, detect_every, iou, follow_grid,
                                                     follow_radius, max_batch, p.device)
    rows = [b for tr in tracks for b in tr]
    offsets = [0] + [int(v) for v in np.cumsum([len(tr) for tr in tracks])]
    n = len(rows)
    res = {"tracks": tracks, "boxes": rows, "track_offsets": offsets, "windows": [], "track_verdicts": [],
           "verdict": (None, None), "segments": []}
    gained = {"follow": moved, "extend": extended, "cuts": cuts, "cut_scores": cut_scores, "transitions": transitions,
              "transition_info": transition_info, "quality": measures}
    res.update({k: v for k, v in gained.items() if v is not None})     # the scores and the info only where computed here
    if n == 0:
        res["frame_scores"] = torch.empty((0, 2), dtype=torch.float32, device=p.device)
        res["window_means"] = torch.empty((0, 2), dtype=torch.float32, device=p.device)
        if opt.persons:
            res["persons"] = {"tracks": [], "of_track": [], "verdicts": [], "distance": np.empty((0, 0), dtype=np.int64),
                              "means": torch.empty((0, 2), dtype=torch.float32, device=p.device), "rows": [],
                              "measured": np.zeros(0, dtype=bool)}
        return res
    if eps is not None and eps.shape[0] != n:
        raise ValueError(f"scan_frames: eps holds {eps.shape[0]} rows for {n} crops")
    with torch.no_grad():
        logits, nets = _scan_logits(fr, model, rows, eps, max_batch)
        voted = _scan_votes(tracks, offsets, logits, nets, window, stride)
        if opt.persons:
            res["persons"] = _scan_persons(fr, tracks, rows, offsets, logits, nets, max_batch, p.device, **opt.pargs)
    res.update(voted)
    return res


def _read_frames(vid, select):
    """The frames ``select(number of frames)`` of the video file ``vid`` as (uint8 (n,H,W,3) RGB, their indices) — decord,
    on the CPU (third-party, imported lazily)."""
    from decord import VideoReader, cpu
    vr = VideoReader(vid, ctx=cpu(0))
    index = list(select(len(vr)))
    return vr.get_batch(index).asnumpy(), index


def read_yuv420(file_or_path, H, W, layout="i420", max_frames=None, **colour):
    """A raw YUV 4:2:0 stream as a ``YUV420``: what ``-pix_fmt yuv420p|nv12 -f rawvideo`` writes, frames of 3HW/2 bytes back
    to back with no header, so ``H``, ``W`` (even) and ``layout`` are the caller's to know.  ``file_or_path``: a path
    (``numpy.fromfile``) or an open binary file object such as a decoder's pipe (``read`` until the end, or until
    ``max_frames`` frames); ``colour``: ``matrix`` and ``full_range`` as ``YUV420`` takes them.  A stream that ends inside a
    frame is a ``GenConViTHipError``; an empty one gives F = 0.  The frames stay on the host: the scan uploads them group
    by group."""
    if not (_is_whole(H) and _is_whole(W) and H >= 2 and W >= 2 and H % 2 == 0 and W % 2 == 0):
        raise _lib.GenConViTHipError(f"read_yuv420: H {H} and W {W} must be even integers of at least 2")
    if max_frames is not None and (not _is_whole(max_frames) or max_frames < 0):
        raise _lib.GenConViTHipError(f"read_yuv420: max_frames {max_frames} must be None or an integer >= 0")
    _lib._check_yuv_names("read_yuv420", layout, colour.get("matrix", "bt709"))
    size = 3 * int(H) * int(W) // 2
    want = -1 if max_frames is None else int(max_frames) * size
    if isinstance(file_or_path, (str, bytes, os.PathLike)):
        data = np.fromfile(file_or_path, dtype=np.uint8, count=want)
    else:
        parts, got = [], 0
        while want < 0 or got < want:                       # a pipe may hand over less than was asked for
            piece = file_or_path.read(-1 if want < 0 else want - got)
            if not piece:
                break
            parts.append(piece)
            got += len(piece)
        data = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    if data.size % size:
        raise _lib.GenConViTHipError(f"read_yuv420: the stream holds {data.size} bytes, {data.size // size} frames of "
                                     f"{size} bytes ({H}x{W}) and a partial one of {data.size % size}")
    return YUV420(data.reshape(-1, 3 * int(H) // 2, int(W)), layout, **colour)


def scan_video(vid, model, every=1, max_frames=None, **kw):
    """``scan_frames`` on the frames ``range(0, len, every)[:max_frames]`` of the video file ``vid``; the result also
    holds ``frame_index``, the source frame number of each scanned frame (the frame numbers in ``tracks``, ``windows``
    and ``segments`` count scanned frames: look them up there).  The file is decoded to RGB on the CPU by third-party
    code (decord); the route without that conversion is ``scan_frames(read_yuv420(pipe, H, W), ...)`` on a decoder's raw
    ``yuv420p`` / ``nv12`` output."""
    if every < 1:
        raise ValueError(f"scan_video: every {every} must be at least 1")
    frames, index = _read_frames(vid, lambda n: list(range(0, n, every))[:max_frames])
    res = scan_frames(frames, model, **kw)
    res["frame_index"] = [int(i) for i in index]
    return res


RENDER_NO_SCORE, RENDER_QUIET, RENDER_FAKE = 0x404040, 0x202020, 0x0000FF     # packed r | g << 8 | b << 16


def _render_plan(what, fr, res, label, eps, lut, thick, strip, max_frames, max_batch, which):
    """The checks of ``render_scan``, all before anything runs, and everything it draws that does not need a device: returns
    ``(rows, marks, timeline, strip, evidence)`` — the crop rows, one mark per row (``gcv_scan_annotate``'s 8 columns, frame
    numbers of the whole video), the (2, F) int64 timeline, the strip height, and the sorted indices of the rows inside a
    FAKE segment of their track."""
    nf, h, w = (int(v) for v in fr.shape[:3])
    need = ("boxes", "track_offsets", "frame_scores", "segments")
    if not isinstance(res, dict) or any(k not in res for k in need):
        raise ValueError(f"{what}: res must be the dict scan_frames returned, with {', '.join(need)}")
    if label not in ("track", "person", None):
        raise ValueError(f"{what}: unknown label {label!r}: accepted values are 'track', 'person' and None")
    if label == "person" and "persons" not in res:
        raise ValueError(f"{what}: label='person' needs res['persons'] (scan_frames(..., persons=True))")
    if which not in ("ed", "vae", "mean"):
        raise ValueError(f"unknown map {which!r}: accepted values are 'ed', 'vae' and 'mean'")
    for name, v in (("max_frames", max_frames), ("max_batch", max_batch)):
        if not _is_whole(v) or v < 1:
            raise ValueError(f"{what}: {name} {v} must be an integer >= 1")
    rows = [tuple(int(v) for v in b) for b in res["boxes"]]
    offsets = [int(v) for v in res["track_offsets"]]
    n, scores = len(rows), res["frame_scores"]
    if not offsets or offsets[0] != 0 or offsets[-1] != n or any(a > b for a, b in zip(offsets, offsets[1:])):
        raise ValueError(f"{what}: res['track_offsets'] does not partition the {n} crop rows")
    if not (torch.is_tensor(scores) and scores.dim() == 2 and scores.shape[0] == n and (n == 0 or scores.shape[1] >= 1)):
        raise ValueError(f"{what}: res['frame_scores'] must hold one row per crop row ({n})")
    for i, b in enumerate(rows):
        if len(b) != 5 or not 0 <= b[0] < nf:
            raise ValueError(f"{what}: crop row {i} is not (frame, top, right, bottom, left) on one of the {nf} frames")
    if eps is not None and eps.shape[0] != n:
        raise ValueError(f"{what}: eps holds {eps.shape[0]} rows for {n} crops")
    if thick is None:
        thick = min(16, max(1, min(h, w) // 240))
    if not _is_whole(thick) or not 1 <= thick <= _lib.ANNOTATE_THICK_MAX:
        raise ValueError(f"{what}: thick {thick} must be an integer in 1 ... {_lib.ANNOTATE_THICK_MAX}")
    if strip is None:
        strip = min(h, max(4, h // 36)) if h >= 2 else 0
    if not _is_whole(strip) or not (strip == 0 or 2 <= strip <= h):
        raise ValueError(f"{what}: strip {strip} must be 0 or an integer in 2 ... {h}: two lanes, one row each at the least")
    ntracks = len(offsets) - 1
    track_of = [t for t in range(ntracks) for _ in range(offsets[t + 1] - offsets[t])]
    names = list(range(ntracks)) if label == "track" else [int(v) for v in res["persons"]["of_track"]] if label == "person" \
        else [-1] * ntracks
    if len(names) != ntracks:
        raise ValueError(f"{what}: res['persons']['of_track'] holds {len(names)} entries for {ntracks} tracks")
    lut = (_lib.jet_lut() if lut is None else lut).cpu().to(torch.int64)
    if tuple(lut.shape) != (256, 3):
        raise ValueError(f"{what}: lut must be a (256,3) uint8 tensor")
    colours = (lut[:, 0] | lut[:, 1] << 8 | lut[:, 2] << 16).tolist()
    fake = scores[:, 0].float().cpu() if n else torch.empty(0)
    k = torch.round(fake * 255.0).clamp(0, 255).to(torch.int64).tolist()
    marks = [(*rows[i], colours[k[i]], int(thick), names[track_of[i]] if 0 <= names[track_of[i]] <= _lib.ANNOTATE_LABEL_MAX else -1)
             for i in range(n)]
    try:
        _lib._check_marks(what, marks, nf, h, w)
    except _lib.GenConViTHipError as e:
        raise ValueError(str(e)) from None
    timeline =torch.tensor([[RENDER_NO_SCORE] * nf, [RENDER_QUIET] * nf], dtype=torch.int64)
    best = {}
    for i, b in enumerate(rows):                                    # the highest FAKE score on each frame
        best[b[0]] = max(best.get(b[0], 0), k[i])
    for f, kk in best.items():
        timeline[0, f] = colours[kk]
    evidence = set()
    for seg in res["segments"]:
        t, first, last = (int(v) for v in seg[:3])
        if not 0 <= t < ntracks:
            raise ValueError(f"{what}: segment {tuple(seg)} names track {t} of {ntracks}")
        timeline[1, max(first, 0):min(last, nf - 1) + 1] = RENDER_FAKE
        evidence.update(i for i in range(offsets[t], offsets[t + 1]) if first <= rows[i][0] <= last)
    return rows, marks, timeline, int(strip), sorted(evidence)


def render_scan(frames, res, model=None, evidence=True, label="track", eps=None, layer="s3", which="mean", alpha=0.5,
                weighted=True, lut=None, thick=None, strip=None, max_frames=128, max_batch=128, sink=None, out="rgb",
                out_matrix="bt709", out_full_range=False):
    """The result of ``scan_frames`` drawn onto the frames it was run on, for the reviewer of a flagged video.  ``frames``:
    the uint8 (F,H,W,3) RGB frames that were scanned, numpy or a tensor on either device, or a ``YUV420`` (they are not
    changed); ``res``:
    what ``scan_frames`` returned for them — ``boxes``, ``track_offsets``, ``frame_scores`` and ``segments`` are read, and
    ``persons`` for ``label="person"``.  Anything else, a crop row on a frame the video does not have, a ``label`` other than
    "track", "person" or None, and "person" without ``res["persons"]`` are a ValueError before anything runs.  Drawn, by
    ``_lib.scan_annotate`` (``gcv_scan_annotate``, include/genconvit_hip.h), all policy being this function's:
      marks     one per crop row, in the (track, frame) order of ``res["boxes"]``: the box's outline, ``thick`` pixels wide
                (default min(16, max(1, min(H, W) // 240))), in the colour ``lut[k]``, k = round(255 * the row's FAKE score)
                — column 0 of ``frame_scores``, the class ``real_or_fake`` calls FAKE; ``lut``: (256,3) uint8, default
                ``_lib.jet_lut()`` — and in the box's corner the number of its track, or of its person
                (``res["persons"]["of_track"]``) for ``label="person"``; numbers above 999, and ``label=None``, draw no tab
      timeline  the lowest ``strip`` rows of every frame (default min(H, max(4, H // 36)); 0: none), one column span per
                scanned frame, T = F, in two lanes: above, the ``lut`` colour of the highest FAKE score among the crops on
                that frame, 0x404040 where there is none; below, red on the frames inside a segment of any track,
                0x202020 elsewhere; a white cursor marks the frame's own place
      evidence  when ``model`` is given and ``evidence`` is true: for the crop rows inside a FAKE segment of their own track
                (first <= frame <= last for a segment (track, first, last, _)), the Grad-CAM map of a forward of ``model``
                is drawn over the box before the marks, as ``explain_frames`` does: sub-batches of at most ``max_batch``
                rows, each one ``_lib.face_crop_preprocess`` on the group's slab, one ``model.explain(x, eps=their rows of
                eps, upsample=False, layer=layer)`` and one ``_lib.cam_overlay`` of ``_overlay_maps(model, cams, which)``
                with ``alpha``, ``weighted`` and ``lut``.  A sub-batch shorter than ``max_batch`` is filled up to it with
                copies of its last row, whose maps are dropped: the 16-bit networks choose their kernels by batch size,
                and a row's map differs in its last bits between a batch of 2 and a batch of 7 (it does not depend on
                the row's place or on the other rows), so without the fill the drawn frames would depend on how many
                such rows share a group, that is on ``max_frames``.  They do depend on ``max_batch``.  ``eps``:
                (n_crops, latent) in crop order, as ``scan_frames`` takes it.  With ``eps=None`` the VAE draws its own noise: the maps are then those of a fresh forward, not
                of the scan's.  The logits of these forwards are dropped (``reference_logits_dtype`` does not matter).
    Consecutive frames [g, g + ``max_frames``) form a group: one upload of the group's frames, the overlay calls, one
    ``_lib.scan_annotate`` in place, so device memory is bounded by the group.  Every frame is rendered, faceless ones
    included: they carry the timeline.  With ``sink``, ``sink(g, slab)`` is called per group in order with the rendered
    uint8 (m,H,W,3) device tensor (the caller encodes or stores it; the slab is not reused) and None is returned; otherwise
    the rendered frames come back as one uint8 (F,H,W,3) CPU tensor.  With no crop row the frames carry the timeline only
    (they are untouched when ``strip`` is 0) and ``model`` is not called.
    ``out``: "rgb" (the default: all of the above), or "i420" / "nv12" for an encoder that wants YUV 4:2:0 — after
    ``_lib.scan_annotate`` every group goes through one ``_lib.rgb_to_yuv420`` (include/genconvit_hip.h: integer arithmetic,
    each chroma sample from the sum of its 2 x 2 block) and ``sink`` gets, or the call returns, uint8 (m, 3H/2, W): half
    the bytes of the RGB frames on the way back.  The matrix and range are those of ``frames`` when it is a ``YUV420``,
    else ``out_matrix`` ("bt601" or "bt709") and ``out_full_range``.  An unknown ``out`` or ``out_matrix`` and an odd H or W
    with a YUV ``out`` are a ValueError before anything runs.
    Not shown: how accurate the scores are, and whether a Grad-CAM map is faithful to what the network used.  Encoding the
    frames into a video file is the caller's."""
    fr = _as_frames("render_scan", frames)
    nf, h, w = (int(v) for v in fr.shape[:3])
    if out not in ("rgb",) + _lib.YUV_LAYOUTS:
        raise ValueError(f"render_scan: unknown out {out!r}: accepted values are 'rgb', 'i420' and 'nv12'")
    colour = fr.colour if isinstance(fr, YUV420) else {"matrix": out_matrix, "full_range": bool(out_full_range)}
    if out != "rgb":
        if colour["matrix"] not in _lib.YUV_MATRICES:
            raise ValueError(f"render_scan: unknown out_matrix {out_matrix!r}: accepted values are 'bt601' and 'bt709'")
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError(f"render_scan: out={out!r} needs frames of even height and width, not {h}x{w}")
    rows, marks, timeline, strip, rows_ev = _render_plan("render_scan", fr, res, label, eps, lut, thick, strip, max_frames,
                                                         max_batch, which)
    p = next(model.parameters()) if model is not None else None
    dev = p.device if p is not None else fr.device if fr.is_cuda else torch.device(device)
    if model is None or not evidence:
        rows_ev = []
    timeline = timeline.to(dev)
    lut = None if lut is None else lut.to(dev)
    done = []
    with torch.no_grad():
        for g in range(0, nf, max_frames):
            m = min(max_frames, nf - g)
            slab = _rgb_slab(fr, slice(g, g + m), dev, copy=True)   # one upload; drawn on in place
            ids = [i for i in rows_ev if g <= rows[i][0] < g + m]
            for s in range(0, len(ids), max_batch):
                sub = ids[s:s + max_batch]
                full = sub + sub[-1:] * (max_batch - len(sub))      # always max_batch rows: see the docstring
                boxes = [(rows[i][0] - g, *rows[i][1:]) for i in full]
                x = _lib.face_crop_preprocess(slab, boxes, dtype=p.dtype)
                noise = None if eps is None else eps[torch.as_tensor(full, device=eps.device)].to(dev)
                _, cams = model.explain(x, eps=noise, upsample=False, layer=layer)
                _lib.cam_overlay(slab, boxes[:len(sub)], _overlay_maps(model, cams, which)[:len(sub)], alpha, weighted, lut,
                                 out=slab)
            here = [(mk[0] - g, *mk[1:]) for mk in marks if g <= mk[0] < g + m]
            _lib.scan_annotate(slab, list(range(g, g + m)), here, timeline if strip else None, strip, out=slab)
            if out != "rgb":
                slab = _lib.rgb_to_yuv420(slab, out, **colour)
            if sink is not None:
                sink(g, slab)
            else:
                done.append(slab.cpu())
    if sink is not None:
        return None
    if done:
        return torch.cat(done)
    if out == "rgb" and torch.is_tensor(fr):
        return fr.cpu().clone()
    return torch.empty((0, 3 * h // 2, w) if out != "rgb" else (0, h, w, 3), dtype=torch.uint8)


def render_video(vid, model, every=1, max_frames=None, scan=None, **kw):
    """``scan_frames`` and ``render_scan`` on the frames ``range(0, len, every)[:max_frames]`` of the video file ``vid``, read
    once: returns ``(res, rendered)``.  ``scan``: a dict of ``scan_frames``'s keyword arguments; ``kw``: ``render_scan``'s
    (its own ``max_frames`` keeps its default here).  ``res`` also holds ``frame_index``, as ``scan_video``'s does.  An
    ``eps`` is given to each of the two on its own.  Decoding is third-party CPU code (decord) and encoding the rendered
    frames is the caller's.  This route moves RGB both ways; the YUV route is ``read_yuv420`` for the frames and
    ``render_scan(..., out="i420" | "nv12")`` for the way back."""
    if every < 1:
        raise ValueError(f"render_video: every {every} must be at least 1")
    frames, index = _read_frames(vid, lambda n: list(range(0, n, every))[:max_frames])
    res = scan_frames(frames, model, **(scan or {}))
    res["frame_index"] = [int(i) for i in index]
    return res, render_scan(frames, res, model, **kw)


def df_face(vid, num_frames, net):
    img = extract_frames(vid, num_frames)
    face, count = face_rec(img)
    return preprocess_frame(face) if count > 0 else []


def is_video(vid):
    return os.path.isfile(vid) and vid.endswith((".avi", ".mp4", ".mpg", ".mpeg", ".mov"))


def set_result():
    return {"video": {"name": [], "pred": [], "klass": [], "pred_label": [], "correct_label": []}}


def store_result(result, filename, y, y_val, klass, correct_label=None, compression=None):
    v = result["video"]
    v["name"].append(filename)
    v["pred"].append(y_val)
    v["klass"].append(klass.lower())
    v["pred_label"].append(real_or_fake(y))
    if correct_label is not None:
        v["correct_label"].append(correct_label)
    if compression is not None:
        v["compression"].append(compression)
    return result
