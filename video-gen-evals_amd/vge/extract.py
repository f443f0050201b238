"""Extraction drivers around the GPU extractors: the callers and on-disk formats either side of them.

Mirrors the reference's extraction scripts, minus video container decoding (cv2 is not part of this framework): callers
pass decoded uint8 RGB frames, or point extract_frame_tree / `python -m vge.extract` at the JPEG frame folders the
reference writes (vge.frames decodes them on the GPU):

  mesh_generator.py:101-145   the TokenHMR front end: person detection (detectron2 Faster R-CNN X101-32x8d-FPN,
                              vge.frcnn), the single-person gate (exactly one person instance with score > 0.5 per
                              frame, >= 80 % of the frames), ViTDetDataset's crop (vge_hmr_crop)

  extract_mesh.py:12-43       mesh_info_to_arrays / save_video_npz -- one np.savez_compressed per video with
                              pose / betas / global_orient / vit / frame_idx / meta (JSON string); the file the scorer's
                              npz reader (vge.ingest, utils.py:383-424) consumes
  mesh_generator.py:101-117   the single-person gate: a frame is used only with exactly one person box; a video with
                              fewer than 80 % such frames is rejected (process_video returns False)
  extract_mesh.py:157-246     per video: process_video -> save_video_npz under <out_root>/<action>/<stem>.npz, or the
                              video goes to the not-single list
  process_video.py:59-91      per video: keypoints.npy [T', 120] float32 under <root>/<action>/<stem>/

The per-frame models run on the GPU (vge.hmr.HmrExtractor, vge.dwpose.Wholebody); nothing here computes features.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Dict, Optional, Sequence, Union

import numpy as np

SINGLE_PERSON_MIN_FRACTION = 0.8   # mesh_generator.py:116 (len(valid_frames) < 0.8 * len(frames) -> False)
PERSON_SCORE_THRESH = 0.5          # mesh_generator.py:107 (pred_classes == 0) & (scores > 0.5): vge_frcnn's gate_thresh


def mesh_info_to_arrays(mesh_info: dict):
    """extract_mesh.py:12-23: {frame_idx: {pose, betas, global_orient, vit}} -> float32 arrays in frame order."""
    frame_ids = sorted(mesh_info.keys())
    pose = np.stack([mesh_info[i]["pose"] for i in frame_ids]).astype(np.float32)
    betas = np.stack([mesh_info[i]["betas"] for i in frame_ids]).astype(np.float32)
    gori = np.stack([mesh_info[i]["global_orient"] for i in frame_ids]).astype(np.float32)
    vit = np.stack([mesh_info[i]["vit"] for i in frame_ids]).astype(np.float32)
    return pose, betas, gori, vit, np.asarray(frame_ids, dtype=np.int32)


def save_video_npz(video_id: str, mesh_info: dict, out_root: Union[str, Path] = "meshes_npz",
                   meta: Optional[dict] = None) -> str:
    """extract_mesh.py:25-43: <out_root>/<dirname(video_id)>/<basename(video_id)>.npz, np.savez_compressed."""
    pose, betas, gori, vit, frames = mesh_info_to_arrays(mesh_info)
    out_dir = Path(out_root) / Path(video_id).parent
    out_dir.mkdir(parents=True, exist_ok=True)
    out_path = out_dir / f"{Path(video_id).name}.npz"
    np.savez_compressed(out_path, pose=pose, betas=betas, global_orient=gori, vit=vit, frame_idx=frames,
                        meta=json.dumps(meta or {}, ensure_ascii=False))
    return str(out_path)


def single_person_frames(person_counts: Sequence[int]) -> Optional[np.ndarray]:
    """mesh_generator.py:101-117: indices of the frames with exactly one person box, or None when there are none
    or fewer than 80 % of the frames qualify (the reference's `return False`)."""
    counts = np.asarray(person_counts)
    valid = np.flatnonzero(counts == 1)
    if valid.size == 0 or valid.size < SINGLE_PERSON_MIN_FRACTION * counts.size:
        return None
    return valid


def gate_videos(keep: np.ndarray, frames_per_video: int, frame_off: int = 0):
    """mesh_generator.py:101-117 over a batch of equal-length videos laid out back to back: keep [n_videos * T] per-frame
    single-person flags -> (accepted video indices, kept frame indices into the batch, descriptor rows
    {frame_off, n_frames, kp_off, kp_frames} of the accepted videos' frame-store entries: the npz holds the kept frames
    only (compacted from `frame_off` on, extract_mesh.py:35-43), keypoints.npy every frame (process_video.py))."""
    keep = np.asarray(keep, bool)
    T = int(frames_per_video)
    nv = keep.size // T
    acc, kept, desc = [], [], []
    off = int(frame_off)
    for v in range(nv):
        valid = single_person_frames(np.where(keep[v * T:(v + 1) * T], 1, 0))
        if valid is None:
            continue
        acc.append(v)
        kept.append(valid + v * T)
        desc.append((off, valid.size, v * T, T))
        off += valid.size
    kept_idx = np.concatenate(kept) if kept else np.zeros(0, np.int64)
    return np.asarray(acc, np.int64), kept_idx, np.asarray(desc, np.int32).reshape(-1, 4)


def gate_mask(n_person) -> np.ndarray:
    """mesh_generator.py:103-111 per frame: exactly one (pred_classes == 0) & (scores > 0.5) instance of the gate
    detector (vge.frcnn.FrcnnDetector's n_person)."""
    return np.asarray(n_person).reshape(-1) == 1


def tokenhmr_front(detector, frames, detections=None):
    """TokenHMRMeshGenerator.process_video's front end (mesh_generator.py:101-145) on the device: detectron2's Faster
    R-CNN X101-32x8d-FPN on every frame (vge.frcnn.FrcnnDetector, the reference's det2_predictor), the per-frame
    single-person gate, the 80 % rule, and ViTDetDataset's crop of every kept frame around its one person box.
    frames: uint8 [F, H, W, 3] RGB on the device; detections: optional (person boxes [F, 4] -- the first class-0
    instance of each frame --, n_person [F]) host arrays already computed for these frames.  Returns (kept frame
    indices, uint8 crops [n, 256, 256, 3] on the device), or None when the reference rejects the video
    (process_video returns False)."""
    from .hmr import crop_persons
    if detections is None:
        out = detector.detect(frames)
        boxes, npers = out["person"][:, 0, :4].cpu().numpy(), out["n_person"].cpu().numpy()
    else:
        boxes, npers = np.asarray(detections[0], np.float32).reshape(-1, 4), np.asarray(detections[1])
    keep = np.flatnonzero(gate_mask(npers))
    F = int(frames.shape[0])
    if keep.size == 0 or keep.size < SINGLE_PERSON_MIN_FRACTION * F:
        return None
    return keep, crop_persons(frames, boxes[keep], keep)


def process_video_frames(hmr, detector, frames, detections=None):
    """TokenHMRMeshGenerator.process_video (mesh_generator.py:91-171) from full frames: front end (detector, gate,
    crops) then TokenHMR on the kept frames -> {frame_idx: {pose [23,3,3], betas, global_orient [1,3,3], vit}} or
    False."""
    front = tokenhmr_front(detector, frames, detections)
    if front is None:
        return False
    idx, crops = front
    out = {k: v.cpu().numpy() for k, v in hmr.extract(crops).items()}
    return {int(f): {"pose": out["pose"][j].reshape(23, 3, 3), "betas": out["betas"][j],
                     "global_orient": out["global_orient"][j].reshape(1, 3, 3), "vit": out["vit"][j]}
            for j, f in enumerate(idx)}


def process_video(hmr, crops, person_counts: Optional[Sequence[int]] = None):
    """MeshGenerator.process_video: TokenHMR on the single-person frames' crops -> mesh_info {frame_idx: {...}}, or
    False for a rejected video.  crops: uint8 [F, 256, 256, 3] RGB person crops on the device (one per frame; the
    box crop / ViTDetDataset warp is upstream), person_counts: detector boxes per frame (None = every frame has
    exactly one person)."""
    import torch
    F = int(crops.shape[0])
    idx = np.arange(F) if person_counts is None else single_person_frames(person_counts)
    if idx is None or F == 0:
        return False
    sel = crops if idx.size == F else crops[torch.as_tensor(idx, device=crops.device)]
    out = {k: v.cpu().numpy() for k, v in hmr.extract(sel).items()}
    return {int(f): {"pose": out["pose"][j].reshape(23, 3, 3), "betas": out["betas"][j],
                     "global_orient": out["global_orient"][j].reshape(1, 3, 3), "vit": out["vit"][j]}
            for j, f in enumerate(idx)}


def keypoint_rows(wholebody, frames) -> np.ndarray:
    """process_video.py:71-84 for one video: DWposeDetector + flatten_first_person_no_padding on every frame ->
    float32 [T', 120] (with the whole-frame fallback every frame yields a row)."""
    return np.asarray(wholebody(frames).cpu().numpy(), dtype=np.float32)


def save_keypoints(rows: np.ndarray, root: Union[str, Path], action: str, vid_id: str) -> str:
    """process_video.py:68, 83-85: <root>/<action>/<vid_id>/keypoints.npy."""
    out = Path(root) / action / vid_id / "keypoints.npy"
    out.parent.mkdir(parents=True, exist_ok=True)
    np.save(out, np.asarray(rows, dtype=np.float32))
    return str(out)


def extract_video(hmr, wholebody, frames, crops, action: str, video: str, mesh_root, kp_root,
                  person_counts: Optional[Sequence[int]] = None, source_path: str = "",
                  detector=None) -> Dict[str, Optional[str]]:
    """One video of extract_mesh.py:main + process_video.py: npz (or None when the single-person gate rejects the
    video, the reference's not-single list) and keypoints.npy paths.  crops None: the TokenHMR front end runs on the
    full frames with `detector` (a vge.frcnn.FrcnnDetector: process_video_frames); otherwise crops are ready-made person
    crops.  DWPose (`wholebody`) runs its own YOLOX-L persons on every frame, as process_video.py does."""
    stem = Path(video).stem
    if crops is None:
        if detector is None:
            raise ValueError("extract_video: the TokenHMR front end needs the gate detector (vge.frcnn.FrcnnDetector)")
        mesh_info = process_video_frames(hmr, detector, frames)
    else:
        mesh_info = process_video(hmr, crops, person_counts)
    npz = None
    if mesh_info:
        npz = save_video_npz(str(Path(action) / stem), mesh_info, out_root=mesh_root,
                             meta={"action": action, "video": video, "source_path": source_path})
    kp = save_keypoints(keypoint_rows(wholebody, frames), kp_root, action, stem)
    return {"npz": npz, "keypoints": kp}


def _pack_passes(items, max_frames: int):
    """The packing rule of extract_videos: items are (key, payload, n_frames) in order; consecutive items go into passes
    of at most `max_frames` frames, a longer one is a pass of its own."""
    passes, cur, n = [], [], 0
    for it in items:
        t = int(it[2])
        if cur and n + t > max_frames:
            passes.append(cur)
            cur, n = [], 0
        cur.append(it)
        n += t
    if cur:
        passes.append(cur)
    return passes


def _run_pass(hmr, wholebody, detector, group, want_kp=None, crop=None):
    """One pass of extract_videos / extract_frame_tree: group is [(key, uint8 [T, H, W, 3] device frames)]; the gate
    detector and DWPose run once over all its frames, TokenHMR once over the crops of every kept frame of the accepted
    videos.  want_kp: per video, whether keypoints are needed (None: all); crop: the person-crop function (None:
    vge.hmr.crop_persons).  Returns per video (key, keypoint rows [T, 120] or None, kept frame indices or None for a
    rejected video, {pose, betas, global_orient, vit} rows of the kept frames or None)."""
    import torch
    if crop is None:
        from .hmr import crop_persons as crop
    fr = group[0][1] if len(group) == 1 else torch.cat([f for _, f in group], 0)
    det = detector.detect(fr)
    lens = [int(f.shape[0]) for _, f in group]
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    want = [True] * len(group) if want_kp is None else [bool(w) for w in want_kp]
    kp_rows = [None] * len(group)
    if all(want):
        kp = wholebody(fr).cpu().numpy()
        kp_rows = [kp[starts[i]:starts[i + 1]] for i in range(len(group))]
    elif any(want):
        sel = [i for i, w in enumerate(want) if w]
        kp = wholebody(torch.cat([group[i][1] for i in sel], 0)).cpu().numpy()
        o = 0
        for i in sel:
            kp_rows[i] = kp[o:o + lens[i]]
            o += lens[i]
    boxes = det["person"][:, 0, :4].cpu().numpy()
    npers = det["n_person"].cpu().numpy()
    kept, valids = [], []
    for i in range(len(group)):
        f0, t = int(starts[i]), lens[i]
        valid = single_person_frames(np.where(gate_mask(npers[f0:f0 + t]), 1, 0))
        valids.append(valid)
        if valid is not None:
            kept.append(valid + f0)
    rows = None
    if kept:
        kf = np.concatenate(kept)
        crops = crop(fr, boxes[kf], kf)
        rows = {k: v.cpu().numpy() for k, v in hmr.extract(crops).items()}
    out, r = [], 0
    for i, (key, _) in enumerate(group):
        valid = valids[i]
        if valid is None:
            out.append((key, kp_rows[i], None, None))
            continue
        out.append((key, kp_rows[i], valid, {k: rows[k][r:r + valid.size] for k in ("pose", "betas", "global_orient",
                                                                                  "vit")}))
        r += valid.size
    return out


def _mesh_info(frame_ids, rows) -> dict:
    return {int(fi): {"pose": rows["pose"][j].reshape(23, 3, 3), "betas": rows["betas"][j],
                      "global_orient": rows["global_orient"][j].reshape(1, 3, 3), "vit": rows["vit"][j]}
            for j, fi in enumerate(frame_ids)}


def extract_videos(hmr, wholebody, detector, videos, mesh_root, kp_root, max_frames: int = 1024,
                   jpeg_quality: Optional[int] = None, frame_cache=None) -> Dict[str, Optional[str]]:
    """extract_mesh.py:150-241 + process_video.py:59-94 over a list of videos, batched for the GPU: videos are
    (stem, uint8 [T, H, W, 3] device frames) of any lengths; consecutive videos are packed into passes of at most
    `max_frames` frames (a longer video is a pass of its own), and each pass runs the gate detector (detectron2 Faster
    R-CNN, `detector`) and DWPose (`wholebody`: YOLOX-L persons -> RTMPose-l) once over all its frames, then TokenHMR
    once over the crops of every kept frame of the pass's accepted videos.  Per video, as the reference does one at a
    time: the single-person gate and its 80 % rule (mesh_generator.py:101-117), <mesh_root>/<stem>.npz of the kept
    frames (extract_mesh.py:35-43; a rejected video gets none: the not-single list) and
    <kp_root>/<stem>/keypoints.npy of every frame (process_video.py writes them for every video).
    jpeg_quality: None hands the frames to the models as they are; a quality (the reference's is 95) first sends each
    pass's frames through vge.frames.jpeg_roundtrip on their device, so the gate detector, DWPose and the person crops
    see the pixels the reference's models see, which only ever read frames back from its JPEG cache
    (extract_mesh.py:47-82, 200-209: cv2.imwrite, then cv2.imread).
    frame_cache: when given, each video's frames are also written to <frame_cache>/<stem>/frame_%06d.jpg at
    `jpeg_quality` (95 when that is None) by vge.frames.save_frames -- GPU frames are Huffman-coded on the device, CPU
    frames on the host -- so an in-memory extraction leaves the cache extract_frame_tree and the reference's
    extract_mesh.py resume from.
    Returns {stem: npz path or None}."""
    out: Dict[str, Optional[str]] = {}
    if frame_cache is not None:
        from .frames import save_frames
        videos = list(videos)
        for stem, fr in videos:
            save_frames(fr, Path(frame_cache) / stem, quality=95 if jpeg_quality is None else jpeg_quality,
                        entropy="device" if fr.device.type == "cuda" else "host")
    for group in _pack_passes([(stem, fr, int(fr.shape[0])) for stem, fr in videos], max_frames):
        members = [(s, f) for s, f, _ in group]
        if jpeg_quality is not None:
            from .frames import jpeg_roundtrip
            members = [(s, jpeg_roundtrip(f, quality=jpeg_quality)) for s, f in members]
        for stem, kp, valid, rows in _run_pass(hmr, wholebody, detector, members):
            save_keypoints(kp, Path(kp_root), "", stem)
            if valid is None:
                out[stem] = None
                continue
            out[stem] = save_video_npz(stem, _mesh_info(valid, rows), out_root=mesh_root, meta={"video": stem})
    return out


# ---- the reference's extraction driver over frame folders (extract_mesh.py:115-241, process_video.py:59-94)

def _load_json(path: Path, default):
    """extract_mesh.py:131-144 load_list / load_dict: a missing or corrupted log starts fresh."""
    if path.exists():
        try:
            with open(path, "r") as f:
                return json.load(f)
        except Exception:
            print(f"[WARN] Corrupted {path}; starting fresh.")
    return default


def _save_json(path: Path, data) -> None:
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w") as f:
        json.dump(data, f, indent=4)


def extract_frame_tree(hmr, wholebody, detector, frames_root, mesh_root, kp_root, log_root, actions=None,
                       max_frames: int = 1024, device=None, threads: int = 0, crop=None,
                       entropy: str = "host", frame_format: str = "jpg",
                       jpeg_quality: Optional[int] = None) -> Dict[str, Dict[str, list]]:
    """extract_mesh.py:150-241 and process_video.py:59-94 together, over the frame folders the reference leaves on
    disk: <frames_root>/<action>/<video>/*.jpg, decoded by vge.frames (the pixels cv2.imread gives the reference).
    frame_format "png" reads <video>/*.png instead: the lossless frames a generator leaves, the array cap.read() would
    have handed to the reference; with jpeg_quality (the reference's is 95) each pass's frames first go through
    vge.frames.jpeg_roundtrip on their device, as in extract_videos, and the models see the reference's pixels.
    frame_format "gif" reads videos that are one animated GIF each, <frames_root>/<action>/<video>.gif (the video name
    is the stem): the frames are the GIF's composed frames (include/vge_gif.h), frame_idx indexes them, pass packing
    uses the probe's frame counts and jpeg_quality applies as for PNG.  A GIF's frames from the first undecodable one
    onward are dropped (they are deltas on it).  frame_format "webp" reads <action>/<video>.webp, one lossless WebP
    file per video (include/vge_webp.h), in exactly the same way, and frame_format "apng" reads <action>/<video>.png
    and <action>/<video>.apng, one animated PNG per video (include/vge_apng.h); when both files exist the .apng is
    used, and a line says so.

    Per action, <log_root>/single/<action>.json and not_single/<action>.json (lists of video names) and
    errors/<action>.json ({video: message}) are rewritten after every video.  A video already in the single or
    not-single list is skipped; one in the error list is tried again (the reference's `processed` set leaves errors
    out).  Keypoints are skipped when <kp_root>/<action>/<video>/keypoints.npy exists (process_video.py:73-76).  A video
    whose folder has no frames, whose frames are all undecodable or whose processing raises gets its message recorded
    under its name and the job goes on.  Videos are packed into passes by extract_videos' rule (on their listed frame
    counts); a pass's videos are decoded in one call and validated before the models see them, and when a pass raises,
    its videos are run again one by one so that one video's failure does not lose the others.

    Outputs: <mesh_root>/<action>/<video>.npz (kept frames only; frame_idx indexes the folder's sorted list of *.jpg
    (or *.png) files, or the GIF's frames, so a frame that failed to decode shows as a gap; meta carries action /
    video / source_path) and
    <kp_root>/<action>/<video>/keypoints.npy.  actions: None (every folder of frames_root), a name or a list of names.
    entropy: where the frames' Huffman decoding (PNG: inflate and unfilter) runs, "host" or "device"
    (vge.frames.load_frames).
    Returns {action: {"single": [...], "not_single": [...], "errors": [...], "skipped": [...]}} for this run."""
    from . import frames as FR
    if frame_format not in ("jpg", "png", "gif", "webp", "apng"):
        raise ValueError(f"frame_format must be 'jpg', 'png', 'gif', 'webp' or 'apng', not {frame_format!r}")
    ext = "." + frame_format
    video_format = FR.VIDEO_FILE_FORMATS.get(frame_format)
    one_file = video_format is not None   # a video is one file
    exts = (".png", ".apng") if frame_format == "apng" else (ext,)   # the later suffix wins when both files exist
    frames_root, log_root = Path(frames_root), Path(log_root)
    all_actions = sorted(d.name for d in frames_root.iterdir() if d.is_dir())
    if actions is None:
        actions = all_actions
    elif isinstance(actions, str):
        actions = [actions]
    for a in actions:
        if a not in all_actions:
            raise ValueError(f"Action '{a}' not found under {frames_root}")   # extract_mesh.py:170-171
    summary: Dict[str, Dict[str, list]] = {}
    for action in actions:
        action_dir = frames_root / action
        if one_file:
            files = [p for p in action_dir.iterdir() if p.is_file() and p.suffix in exts]
            videos = sorted({p.stem for p in files})
            for v in videos:
                if sum(p.stem == v for p in files) > 1:
                    print(f"[WARN] {action}/{v}: both {v}{exts[0]} and {v}{exts[-1]} exist, using {v}{exts[-1]}")
        else:
            videos = sorted(d.name for d in action_dir.iterdir() if d.is_dir())

        def source(video):
            if not one_file:
                return action_dir / video
            found = [e for e in exts if (action_dir / (video + e)).is_file()]
            return action_dir / (video + (found[-1] if found else exts[0]))
        single_path = log_root / "single" / f"{action}.json"
        not_path = log_root / "not_single" / f"{action}.json"
        err_path = log_root / "errors" / f"{action}.json"
        singles, nots = _load_json(single_path, []), _load_json(not_path, [])
        errs = _load_json(err_path, {})
        processed = set(singles) | set(nots)
        done = summary.setdefault(action, {"single": [], "not_single": [], "errors": [], "skipped": []})

        def fail(video, msg):
            print(f"[WARN] Failed on {source(video)}: {msg}")
            errs[video] = msg
            _save_json(err_path, errs)
            done["errors"].append(video)

        def finish(video, frames_kept, kp, valid, rows):
            """Write one video's outputs and move it to its list."""
            if kp is not None:
                save_keypoints(kp, kp_root, action, video)
            if valid is None:
                nots.append(video)
                _save_json(not_path, nots)
                done["not_single"].append(video)
            else:
                save_video_npz(str(Path(action) / video), _mesh_info(frames_kept[valid], rows), out_root=mesh_root,
                               meta={"action": action, "video": video, "source_path": str(source(video))})
                singles.append(video)
                _save_json(single_path, singles)
                done["single"].append(video)
            if errs.pop(video, None) is not None:
                _save_json(err_path, errs)

        todo = []
        for video in videos:
            if video in processed:
                print(f"[SKIP] {action}/{video} (already processed)")
                done["skipped"].append(video)
                continue
            todo.append((video, str(source(video)) if one_file else FR.list_frames(action_dir / video, ext=ext)))
        if one_file:   # a video is one file: the probe gives its frame count
            counts = FR._probe(video_format, [p for _, p in todo], threads)[:, video_format.count_col] if todo else []
            entries = []
            for (v, p), n in zip(todo, counts):
                if int(n) > 0:
                    entries.append((v, p, int(n)))
                else:
                    fail(v, f"no decodable frame in {p}: not a {frame_format.upper()}, truncated, or without an image")
        else:
            entries = [(v, paths, len(paths)) for v, paths in todo]
        for group in _pack_passes(entries, max_frames):
            # decode and validate: one call for the pass; a video that makes it raise is found one by one
            try:
                decoded = FR.load_videos([paths for _, paths, _ in group], device=device, threads=threads,
                                         entropy=entropy)
            except Exception:
                decoded = []
                for _, paths, _ in group:
                    try:
                        decoded.append(FR.load_frames(paths, device=device, threads=threads, entropy=entropy))
                    except Exception as e:
                        decoded.append(e)
            good = []
            for (video, paths, count), dec in zip(group, decoded):
                if isinstance(dec, Exception):
                    fail(video, str(dec))
                elif one_file and dec[1].size == 0:
                    fail(video, f"none of the {count} frames of {paths} could be decoded")
                elif not paths:
                    fail(video, f"no frames (*{ext}) in {action_dir / video}")
                elif dec[1].size == 0:
                    fail(video, f"none of the {len(paths)} frames in {action_dir / video} could be decoded")
                else:
                    fr = dec[0] if jpeg_quality is None else FR.jpeg_roundtrip(dec[0], quality=jpeg_quality)
                    good.append((video, fr, np.asarray(dec[1], np.int64)))
            if not good:
                continue
            # frames of one pass are stacked: consecutive videos of one frame size run together
            runs = []
            for g in good:
                if runs and tuple(runs[-1][-1][1].shape[1:]) == tuple(g[1].shape[1:]):
                    runs[-1].append(g)
                else:
                    runs.append([g])
            for run in runs:
                want_kp = [not (Path(kp_root) / action / v / "keypoints.npy").exists() for v, _, _ in run]
                kept_of = {v: k for v, _, k in run}
                try:
                    results = _run_pass(hmr, wholebody, detector, [(v, f) for v, f, _ in run], want_kp, crop)
                except Exception as e:
                    results = []
                    if len(run) == 1:
                        fail(run[0][0], str(e))
                    else:   # one video's failure must not lose the others of its pass
                        for (v, f, _), w in zip(run, want_kp):
                            try:
                                results += _run_pass(hmr, wholebody, detector, [(v, f)], [w], crop)
                            except Exception as e1:
                                fail(v, str(e1))
                for video, kp, valid, rows in results:
                    try:
                        finish(video, kept_of[video], kp, valid, rows)
                    except Exception as e:
                        fail(video, str(e))
    return summary


def _load_state_dict(path: str) -> Dict[str, np.ndarray]:
    """A checkpoint file -> {name: float array}: torch.load(weights_only=True) of a plain state_dict or of a dict that
    holds one under state_dict / model_state_dict / model (as vge.eval.load_model reads the scorer's)."""
    import torch
    ck = torch.load(path, map_location="cpu", weights_only=True)
    for k in ("model_state_dict", "state_dict", "model"):
        if isinstance(ck, dict) and isinstance(ck.get(k), dict):
            ck = ck[k]
            break
    return {k: v.detach().cpu().numpy() for k, v in ck.items() if isinstance(v, torch.Tensor)}


def main(argv=None) -> int:
    """python -m vge.extract: the reference's extract_mesh.py + process_video.py over a tree of frame folders."""
    import argparse
    ap = argparse.ArgumentParser(
        description="TokenHMR meshes + DWPose keypoints from <frames-root>/<action>/<video>/*.jpg (or *.png), or "
                    "<action>/<video>.gif")
    ap.add_argument("--frames-root", required=True)
    ap.add_argument("--mesh-root", required=True)
    ap.add_argument("--kp-root", required=True)
    ap.add_argument("--log-root", required=True)
    ap.add_argument("--action", default=None,
                    help="Optional: only process this action (directory name). If not set, process all actions.")
    ap.add_argument("--hmr-ckpt", help="TokenHMR state_dict")
    ap.add_argument("--frcnn-ckpt", help="detectron2 Faster R-CNN X101-32x8d-FPN state_dict (the single-person gate)")
    ap.add_argument("--yolox-ckpt", help="DWPose's YOLOX-L state_dict")
    ap.add_argument("--rtmpose-ckpt", help="DWPose's RTMPose-l whole-body state_dict")
    ap.add_argument("--synthetic-weights", action="store_true",
                    help="deterministic random weights of the full-size models (vge.synth), for dry runs")
    ap.add_argument("--max-frames", type=int, default=1024, help="frames per GPU pass")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--threads", type=int, default=0, help="frame decode threads (0: the ingest default)")
    ap.add_argument("--entropy", choices=("host", "device"), default="host",
                    help="where the frames' Huffman decoding (PNG: inflate and unfilter) runs (vge.frames.load_frames)")
    ap.add_argument("--frame-format", choices=("jpg", "png", "gif", "webp", "apng"), default="jpg",
                    help="the frame files each video folder holds; gif / webp / apng: each video is one animated "
                         "<video>.gif, lossless <video>.webp or animated <video>.png / <video>.apng")
    ap.add_argument("--jpeg-quality", type=int, default=None,
                    help="send the decoded frames through a JPEG round trip of this quality before the models "
                         "(the reference's cache is 95; meant for PNG frames)")
    args = ap.parse_args(argv)
    from . import synth
    from .dwpose import RTMPOSE_L, YOLOX_L, DwposeExtractor, Wholebody, YoloxDetector
    from .frcnn import FRCNN_X101, FrcnnDetector
    from .hmr import TOKENHMR, HmrExtractor

    def weights(path, make, what):
        if path:
            return _load_state_dict(path)
        if args.synthetic_weights:
            return make()
        ap.error(f"--{what}-ckpt is required (or --synthetic-weights)")

    dev, fc = args.device, args.max_frames
    hmr = HmrExtractor(weights(args.hmr_ckpt, lambda: synth.make_hmr_state_dict(TOKENHMR), "hmr"), TOKENHMR,
                       device=dev, max_frames=fc)
    gdet = FrcnnDetector(weights(args.frcnn_ckpt, lambda: synth.make_gate_frcnn_state_dict(FRCNN_X101), "frcnn"),
                         FRCNN_X101, device=dev, chunk=128)
    wb = Wholebody(YoloxDetector(weights(args.yolox_ckpt, lambda: synth.make_gate_detector_state_dict(YOLOX_L), "yolox"),
                                 YOLOX_L, device=dev, chunk=256),
                   DwposeExtractor(weights(args.rtmpose_ckpt, lambda: synth.make_rtmpose_state_dict(RTMPOSE_L), "rtmpose"),
                                   RTMPOSE_L, device=dev, max_instances=2 * fc))
    summary = extract_frame_tree(hmr, wb, gdet, args.frames_root, args.mesh_root, args.kp_root, args.log_root,
                                 actions=args.action, max_frames=fc, device=dev, threads=args.threads,
                                 entropy=args.entropy, frame_format=args.frame_format,
                                 jpeg_quality=args.jpeg_quality)
    for action, d in summary.items():
        print(f"[DONE] {action}: {len(d['single'])} single, {len(d['not_single'])} not single, "
              f"{len(d['errors'])} errors, {len(d['skipped'])} skipped")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
