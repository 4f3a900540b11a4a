"""What the three ``-process`` paths of handler.Handler share (segment, _segment_fit, _segment_video): the folder listing, the chunk
size, how a shrunk uint8 frame is fed to the network, the PNG columns with their by-position names, and ``-objects`` /
``--track-iou`` on the 64 x 64 masks (objects.json, tracks.json and their PNGs; ``video_reports`` writes the two reports of
``--source-video --overlay-tracks`` without PNGs; with ``--object-value`` the objects are scored by the critic and, with
``--min-value-drop``, selected before they are reported and tracked: {stem}-valued-mask.png), and ``--clean`` (``clean_source``, ``write_clean``: clean.json and the
{stem}-clean-mask.png files), and ``--graph-cut`` (``cut_source``, ``write_cut``: cut.json and the {stem}-cut-mask.png files; the cut
mask then stands where the CRF mask stands, under the name "cut-mask").  Under data parallelism every rank makes the GPU
calls and rank 0 writes."""
import os

import numpy as np
import torch

from . import clean, graphcut, objects
from .evaluate import MATCH_MAX_OBJECTS, write_json

PROCESS_MAX_OBJECTS = 256       # rows of the object table of -process -objects
# one column per output kind, in the reference's order; the file name of a column is its POSITION here (main.py:1212-1223)
KINDS = ("raw-mask", "thresholded-mask", "crf-mask", "saliency-map", "thresholded-saliency", "crf-saliency")


def list_folder(folder):
    """(files, stems) of a folder of frames in os.listdir's order; a name without a dot has no stem."""
    files = os.listdir(folder)
    return files, [f.rsplit(".", 1)[0] for f in files if "." in f]


def chunk_frames(max_frames, max_bytes, H, W):
    """Frames per chunk of H x W RGB frames: at most max_frames and about max_bytes, at least one."""
    return max(1, min(max_frames, max_bytes // (3 * H * W)))


def unit_table(device):
    """float32(k / 255.0) for the 256 byte values, rounded on the host as the plain path rounds its frames: the device's own fp32
    division is not correctly rounded, so low.float() / 255 would differ from it in the last bit for some k."""
    return torch.from_numpy((np.arange(256) / 255.0).astype(np.float32)).to(device)


def fit_infer(eng, low, unit, fp16, train_mode):
    """The masks Z [n,64,64] of the shrunk uint8 frames `low`, as -process runs 64 x 64 frames: the fp16 layers take the bytes, the
    fp32 ones the unit_table values (train_mode: -noevalmode, Dropout stays on)."""
    if fp16:
        return eng.infer(low, fp16=True)[1]
    return eng.infer(unit[low.long()], train_mode=train_mode)[1]


def write_columns(out_dir, stems, frames, cols, concatenated):
    """The PNGs of a run of frames: frames uint8 [n,H,W,3], cols a list of grey uint8 stacks [n,H,W] in KINDS' order.  -concatenated:
    frame | column 1 | column 2 ... side by side as {stem}_with_mask.png, else one {stem}-{kind}.png per column."""
    from PIL import Image
    rgb = lambda a: np.repeat(a[:, :, None], 3, axis=2)
    for i, stem in enumerate(stems):
        if concatenated:
            Image.fromarray(np.concatenate([frames[i]] + [rgb(c[i]) for c in cols], axis=1)).save(f"{out_dir}/{stem}_with_mask.png")
        else:
            for kind, c in zip(KINDS, cols):
                Image.fromarray(rgb(c[i])).save(f"{out_dir}/{stem}-{kind}.png")


def binary_source(args, M, crf_mask, device, cleaned=None, hard="crf-mask"):
    """The stack -objects and --track-iou describe: (source name, threshold, device stack, objects.label's keywords) -- with -crf the
    CRF masks, else M >= --binarymaskthreshold (the comparison of the thresholded column).  cleaned: with --clean the bool stack
    clean_source made of that one; it is handed on under the name "clean-mask" / "clean-crf-mask".  hard: the name of the refined
    stack in crf_mask's place, "cut-mask" with --graph-cut (then "clean-cut-mask")."""
    kw = dict(connectivity=args.connectivity, min_area=args.min_area)
    if cleaned is not None:
        return ("clean-" + hard, None, cleaned, kw) if crf_mask is not None else ("clean-mask", float(args.binarymaskthreshold), cleaned, kw)
    if crf_mask is not None:
        return hard, None, torch.from_numpy(np.ascontiguousarray(crf_mask[:, 0])).to(device), kw
    thresh = float(args.binarymaskthreshold)
    return ("thresholded-mask", thresh, torch.from_numpy(np.ascontiguousarray(M[:, 0], dtype=np.float32)).to(device),
            dict(kw, thresh=thresh, inclusive=True))


def clean_source(args, soft, hard, device, hard_name="crf-mask"):
    """--clean: the stack binary_source names, cleaned on the GPU (clean.clean).  soft: the masks [n,64,64] float32 (array or tensor),
    read as soft >= --binarymaskthreshold; hard: with -crf the CRF labels [n,64,64] bool, which then are the source (with --graph-cut
    the cut masks, hard_name="cut-mask").  Returns (source name, threshold, clean.Cleaned on the device)."""
    to_dev = lambda a, dtype: a.to(device) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)
    kw = clean.spec_kwargs(args.clean)
    if hard is not None:
        return hard_name, None, clean.clean(to_dev(hard, bool), **kw)
    thresh = float(args.binarymaskthreshold)
    return "thresholded-mask", thresh, clean.clean(to_dev(soft, np.float32), thresh=thresh, inclusive=True, **kw)


def write_clean(args, source, thresh, counts, stems, rank, pngs=None):
    """Rank 0 writes {R}/clean.json -- the spec, the source and its threshold, the summed counts and the counts per stem -- and, when
    pngs (uint8 [n,H,W], 0 / 1) is given, per frame {R}/{stem}-clean-mask.png as 0 / 255 grey RGB (not a column: the by-position naming
    and the concatenated strip stay as they are).  counts: int32 [n,8] of clean.clean, tensor or array."""
    if rank != 0:
        return
    out_dir = args.mask_output_imgs
    c = counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    write_json(f"{out_dir}/clean.json", {"source": source, "threshold": thresh, **clean.clean_report(c, args.clean),
                                         "per_frame": {stem: {k: int(v) for k, v in zip(clean.COUNTS, c[i])} for i, stem in enumerate(stems)}})
    if pngs is not None:
        write_clean_pngs(out_dir, stems, pngs)


def write_clean_pngs(out_dir, stems, masks):
    """{R}/{stem}-clean-mask.png of a run of frames: masks uint8 or bool [n,H,W], non-zero = on, written as 0 / 255 grey RGB."""
    from PIL import Image
    for i, stem in enumerate(stems):
        grey = (np.asarray(masks[i]) != 0) * np.uint8(255)
        Image.fromarray(np.repeat(grey[:, :, None], 3, axis=2)).save(f"{out_dir}/{stem}-clean-mask.png")


def cut_source(args, frames, soft, device):
    """--graph-cut: the masks refined by graphcut.cut, seeded as the thresholded column compares (soft >= --binarymaskthreshold).
    frames: uint8 [n,64,64,3], soft: float32 [n,64,64] (arrays or tensors).  Returns (threshold, graphcut.Cut on the device)."""
    to_dev = lambda a, dtype: a.to(device) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)
    thresh = float(args.binarymaskthreshold)
    return thresh, graphcut.cut(to_dev(frames, np.uint8), to_dev(soft, np.float32), thresh, inclusive=True, **graphcut.spec_kwargs(args.graph_cut))


def write_cut(args, thresh, stats, stems, rank, pngs=None):
    """Rank 0 writes {R}/cut.json -- the spec, the source threshold and the band it gives, the summed stats and the stats per stem --
    and, when pngs (uint8 or bool [n,H,W]) is given, per frame {R}/{stem}-cut-mask.png as 0 / 255 grey RGB (not a column: the
    by-position naming and the concatenated strip stay as they are).  stats: int32 [n,8] of graphcut.cut, tensor or array."""
    if rank != 0:
        return
    out_dir = args.mask_output_imgs
    c = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    lo, hi = graphcut.spec_band(args.graph_cut, thresh)
    write_json(f"{out_dir}/cut.json", {"source": "thresholded-mask", "threshold": thresh, "lo": lo, "hi": hi,
                                       **graphcut.cut_report(c, args.graph_cut),
                                       "per_frame": {stem: {k: int(v) for k, v in zip(graphcut.STATS, c[i])} for i, stem in enumerate(stems)}})
    if pngs is not None:
        write_cut_pngs(out_dir, stems, pngs)


def write_cut_pngs(out_dir, stems, masks):
    """{R}/{stem}-cut-mask.png of a run of frames: masks uint8 or bool [n,H,W], non-zero = on, written as 0 / 255 grey RGB."""
    from PIL import Image
    for i, stem in enumerate(stems):
        grey = (np.asarray(masks[i]) != 0) * np.uint8(255)
        Image.fromarray(np.repeat(grey[:, :, None], 3, axis=2)).save(f"{out_dir}/{stem}-cut-mask.png")


def objects_and_tracks(args, M, crf_mask, stems, device, rank, low=None, cleaned=None, infer=None, hard="crf-mask"):
    """-process -objects [--track-iou]: the stack of binary_source labelled on the GPU once (objects.py; labels, mask and counts do not
    depend on the table's rows), then reported as objects and, if asked for, as tracks.  low: with --track-motion the uint8 frames
    [n,64,64,3] the masks were made from (tensor or array, in the order of stems); --track-reid needs them too.  cleaned: with --clean the cleaned bool stack on the
    device, which is then the one described; the reports' header gains "clean".  infer: with --object-value the critic, uint8 frames
    [b,64,64,3] -> values [b] in eval mode; low is then needed too.  The objects 1..64 of every frame are scored (objects.value), and
    with --min-value-drop the ones that pass are what the mask PNGs and the tracks describe (objects.select).  hard: binary_source's."""
    want_tracks = bool(getattr(args, "track_iou", ""))
    want_value = bool(getattr(args, "object_value", False))
    source, thresh, stack, kw = binary_source(args, M, crf_mask, device, cleaned, hard)
    res = objects.label(stack, max_objects=PROCESS_MAX_OBJECTS, want_labels=want_tracks or want_value, want_mask=True, **kw)
    head = {"source": source, "threshold": thresh, "connectivity": args.connectivity, "min_area": args.min_area,
            **({"clean": dict(args.clean)} if cleaned is not None else {}),
            **({"graph_cut": dict(args.graph_cut)} if hard == "cut-mask" else {})}
    valued = drops = None
    if want_value:
        if low is None or infer is None:
            raise ValueError("--object-value needs the 64 x 64 frames of the masks and the critic")
        valued = _valued(args, res, torch.as_tensor(low).to(device), infer, stems)
        res_all, res, drops = res, valued["objects"], valued["drops"]
        _objects(args, res_all, head, stems, M.shape[-1], rank, valued=valued)
    else:
        _objects(args, res, head, stems, M.shape[-1], rank)
    if want_tracks:
        search = int(getattr(args, "track_motion", 0) or 0)
        reid = getattr(args, "track_reid", None)
        if (search or reid) and low is None:
            raise ValueError("--track-motion and --track-reid need the 64 x 64 frames of the masks")
        _tracks(args, res, head, stems, rank, low=torch.as_tensor(low).to(device) if search or reid else None, search=search,
                fill=bool(getattr(args, "track_fill", False)),
                reid=(reid, args.track_reid_window, args.track_reid_area) if reid else None, drops=drops)


def _valued(args, res, frames, infer, stems):
    """--object-value: objects.value of the labelled stack and, with --min-value-drop, objects.select.  Returns {"head": the
    "object_value" header, "base" [n] and "drop" [n,64] (host), "keep" bool [n,64] and "label_selected" int [n,64] (host, None without
    a threshold), "mask": the selected kept-pixel mask (host, None likewise), "objects": the Objects everything downstream describes
    (the selected ones with a threshold, else res), "drops": float64 [n,64], the drop of every object of "objects" by ITS number}."""
    K = MATCH_MAX_OBJECTS
    fill, grow, V = args.object_value_fill, args.object_value_grow, args.min_value_drop
    val = objects.value(infer, frames, res.labels, res.kept, fill=fill, grow=grow, max_objects=K)
    drop = val.drop.cpu().numpy()
    out = {"base": val.base.cpu().numpy(), "drop": drop, "keep": None, "label_selected": None, "mask": None, "objects": res,
           "drops": drop.astype(np.float64)}
    keep = unscored = None
    if V is not None:
        keep = objects.value_keep(val.drop, res.kept, V)
        sel, unscored = objects.select(res, keep)
        keep = keep.cpu().numpy()
        number = np.where(keep, np.cumsum(keep, axis=1), 0)
        drops = np.zeros((len(drop), K), dtype=np.float64)
        for f, k in zip(*np.nonzero(keep)):
            drops[f, number[f, k] - 1] = drop[f, k]
        out.update(keep=keep, label_selected=number, mask=sel.mask.cpu().numpy(), objects=sel, drops=drops)
    out["head"] = objects.value_report(val, res.kept, fill, grow, V, unscored=unscored, stems=stems)
    for key in ("base_mean", "drop"):                                  # (the summary figures are -eval's)
        out["head"].pop(key)
    return out


def video_reports(args, M, stem, device, rank, bwd=None):
    """--source-video --overlay-tracks: the whole-stack reports of the masks M [n,1,64,64] that the stream returned, labelled as the
    stream labelled them (threshold inclusive, 8-connected, --overlay-min-area), as {R}/{stem}-objects.json and {R}/{stem}-tracks.json
    with the frames keyed "000000", "000001", ... in stream order and no PNG.  objects.TrackStream gives objects.track's numbers, so
    the numbers of tracks.json are the ones drawn on the video.  bwd: with --overlay-motion the backward field the stream tracked along,
    int8 [n - 1,8,8,2] on the device.  With --overlay-fill {stem}-tracks.json carries what --track-fill adds to tracks.json (the
    whole stack filled by objects.fill: the stream's objects.FillStream gives the same).  Returns the two file names."""
    thresh = float(args.binarymaskthreshold)
    stack = torch.from_numpy(np.ascontiguousarray(M[:, 0], dtype=np.float32)).to(device)
    res = objects.label(stack, thresh=thresh, inclusive=True, connectivity=8, min_area=args.overlay_min_area,
                        max_objects=PROCESS_MAX_OBJECTS, want_labels=True, want_mask=False)
    head = {"source": "thresholded-mask", "threshold": thresh, "connectivity": 8, "min_area": args.overlay_min_area}
    stems = [f"{i:06d}" for i in range(len(M))]
    names = (f"{stem}-objects.json", f"{stem}-tracks.json")
    _objects(args, res, head, stems, M.shape[-1], rank, png=False, name=names[0])
    _tracks(args, res, head, stems, rank, png=False, name=names[1], iou=args.overlay_tracks, gap=int(getattr(args, "overlay_gap", 0) or 0),
            bwd=bwd, search=int(getattr(args, "overlay_motion", 0) or 0) if bwd is not None else 0,
            fill=bool(getattr(args, "overlay_fill", False)))
    return list(names)


def _objects(args, res, head, stems, width, rank, png=True, name="objects.json", valued=None):
    """Rank 0 writes {R}/objects.json and per frame {R}/{stem}-objects-mask.png, the pixels of the kept objects as 0 / 255 grey RGB
    (png=False: the report alone, as {R}/{name}).  valued (--object-value, _valued's dict): the header gains "object_value", every
    frame "value" (the critic's value of the frame) and every object "value_drop" (None for an object numbered above 64, which is never
    scored); with --min-value-drop every object also "selected" and "label_selected" (its new number, 0 when dropped), the mask PNG
    shows the selected objects and {stem}-valued-mask.png is written from the same mask."""
    from PIL import Image
    if rank != 0:
        return
    kept, found = res.kept.cpu().numpy(), res.found.cpu().numpy()
    rows = objects.table_rows(res.table, kept, width=width)
    frame_more = lambda i: {}
    if valued is not None:
        drop, keep, number = valued["drop"], valued["keep"], valued["label_selected"]
        head = {**head, "object_value": valued["head"]}
        frame_more = lambda i: {"value": float(valued["base"][i])}
        for i, frame in enumerate(rows):
            for row in frame:
                k = row["label"] - 1
                scored = k < drop.shape[1]
                row["value_drop"] = float(drop[i, k]) if scored else None
                if keep is not None:
                    row.update(selected=bool(scored and keep[i, k]), label_selected=int(number[i, k]) if scored else 0)
    out_dir = args.mask_output_imgs
    write_json(f"{out_dir}/{name}", {**head, "max_objects": PROCESS_MAX_OBJECTS, "frames": {
        stem: {"found": int(found[i]), "kept": int(kept[i]), **frame_more(i), "objects": rows[i]} for i, stem in enumerate(stems)}})
    if not png:
        return
    selected = valued is not None and valued["mask"] is not None
    mask = valued["mask"] if selected else res.mask.cpu().numpy()
    for i, stem in enumerate(stems):
        grey = Image.fromarray(np.repeat((mask[i] * np.uint8(255))[:, :, None], 3, axis=2))
        grey.save(f"{out_dir}/{stem}-objects-mask.png")
        if selected:
            grey.save(f"{out_dir}/{stem}-valued-mask.png")


def _tracks(args, res, head, stems, rank, png=True, name="tracks.json", iou=None, gap=None, low=None, bwd=None, search=0, fill=False,
            reid=None, drops=None):
    """The objects objects.json describes followed through the frames in natural order of their names on the GPU (objects.track);
    labels above 64 are untracked.  Rank 0 writes {R}/tracks.json and per frame {R}/{stem}-tracks-mask.png, a colour per track
    (png=False: the report alone, as {R}/{name}; iou, gap: the link threshold and the gap when they are not --track-iou's and
    --track-gap's).  With a gap G > 0 (objects.track's max_gap) the report also holds "track_gap", the summary's and the tracks' gap
    keys and per object its "gap"; "last" is then the track's last frame, missed frames counted.  With search S > 0 (--track-motion,
    --overlay-motion) the labels are carried along the backward block vectors (objects.track's motion): temporal.flow of low, uint8
    [n,64,64,3] in the order of stems, taken in the tracked order, or bwd where the caller has the field; the report gains
    "track_motion" (objects.motion_report).  fill (--track-fill, with a gap): the frames a bridged link jumps over get the tail
    object's carried mask (objects.fill).  {stem}-tracks-mask.png is then painted from the filled labels, {stem}-filled-mask.png holds
    the filled labels > 0 as 0 / 255 grey RGB, and the report gains "track_fill" (objects.fill_report), per frame an entry {"label",
    "track", "filled": the frames the mask was carried over, "area"} for every new object, and per track "filled", the number of its
    new objects, counted on the device.  reid (--track-reid: similarity, window, area): the tracks are chained into identities by the
    colour histograms of low (objects.appearance, objects.reid); the report gains "track_reid" (objects.reid_report), per track
    "identity", "reid_prev" and "reid_sim", and the list "identities", and {stem}-identities-mask.png is painted with
    objects.track_colours of every pixel's identity, from the filled labels with fill.  Nothing else changes.  drops (--object-value):
    float64 [n,64] in the order of stems, the value drop of every object of res by its number; every track row then gains
    "value_drop_mean" and "value_drop_max" over its segmented objects."""
    from PIL import Image
    K, iou = MATCH_MAX_OBJECTS, objects.parse_track_iou(args.track_iou) if iou is None else iou
    gap = int(getattr(args, "track_gap", 0) or 0) if gap is None else gap
    order = objects.natural_order(stems)                             # os.listdir's order is arbitrary; only the label stack is reordered
    pick = torch.tensor(order, dtype=torch.int64, device=res.labels.device)
    if search and bwd is None:
        from . import temporal
        bwd = temporal.flow(low[pick], search)[1]
    fill = bool(fill and gap)
    stack = res.labels[pick]
    tr = objects.track(stack, iou=iou, max_objects=K, want_rgb=png and not fill, max_gap=gap, motion=bwd if search else None)
    if fill:
        fl = objects.fill(stack, tr, motion=bwd if search else None, max_objects=K, want_rgb=png)
        new = fl.age > 0
        per_track = torch.bincount(fl.track[new].to(torch.int64).clamp(min=0), minlength=stack.shape[0] * K + 1)
    if reid:
        rd = objects.reid(tr, objects.appearance(low[pick].contiguous(), stack, tr, max_objects=K), stack.shape[0], *reid)
        painted = fl.labels if fill else stack
        per_object = objects.identities(fl.track if fill else tr.track, rd.identity)
        number = torch.gather(per_object, 1, (painted.reshape(painted.shape[0], -1).to(torch.int64) - 1).clamp(0, K - 1)).reshape(painted.shape)
        identity_rgb = objects.track_colours(torch.where((painted >= 1) & (painted <= K), number, torch.zeros_like(number))) if png else None
    if rank != 0:
        return
    totals = torch.stack([tr.n_tracks, tr.n_links, tr.n_objects, tr.longest])
    more = {"max_gap": gap, "gap_links": tr.gap_links, "missed": tr.extra[:, 1].sum(dtype=torch.int64)} if gap else {}
    side = objects.track_report(totals, tr.table[:, 2], tr.table[:, 6].sum(dtype=torch.int64), tr.table[:, 7].sum(dtype=torch.int64),
                                (res.kept[pick] - K).clamp(min=0).sum(), **more)
    rows = objects.track_rows(tr.table, side["tracks"], tr.extra)
    names = [stems[i] for i in order]
    prev, trk = tr.prev.cpu().numpy(), tr.track.cpu().numpy()
    gaps = tr.gap.cpu().numpy() if gap else None
    last = (lambda r: r["last_frame"]) if gap else (lambda r: r["first_frame"] + r["length"] - 1)
    report = {**head, "max_objects": K, "track_iou": iou, **({"track_gap": gap} if gap else {}),
              **({"track_motion": objects.motion_report(bwd, search)} if search else {}),
              **({"track_fill": objects.fill_report(fl)} if fill else {}), "summary": side, "order": names,
              "frames": {stem: [{"label": int(l) + 1, "track": int(trk[j, l]), "prev": int(prev[j, l]),
                                 **({"gap": int(gaps[j, l])} if gap else {})} for l in np.flatnonzero(trk[j])]
                         for j, stem in enumerate(names)},
              "tracks": [{"track": r["track"], "first": names[r["first_frame"]], "last": names[last(r)],
                          "length": r["length"], "area_sum": r["area_sum"], "area_min": r["area_min"], "area_max": r["area_max"],
                          "link_iou": r["link_iou"], **({"bridges": r["bridges"], "missed": r["missed"]} if gap else {})} for r in rows]}
    if drops is not None:                                            # host float64, over the segmented objects of every track
        members = {}
        for j, l in zip(*np.nonzero(trk)):
            members.setdefault(int(trk[j, l]), []).append(float(drops[order[j], l]))
        for row in report["tracks"]:
            d = np.array(members[row["track"]], dtype=np.float64)
            row.update(value_drop_mean=float(d.mean()), value_drop_max=float(d.max()))
    if fill:
        age, ftrk, area, per_track = fl.age.cpu().numpy(), fl.track.cpu().numpy(), fl.table[:, :, 0].cpu().numpy(), per_track.cpu().numpy()
        for j, stem in enumerate(names):
            report["frames"][stem] += [{"label": int(l) + 1, "track": int(ftrk[j, l]), "filled": int(age[j, l]), "area": int(area[j, l])}
                                       for l in np.flatnonzero(age[j])]
        for row in report["tracks"]:
            row["filled"] = int(per_track[row["track"]])
    if reid:
        identity, r_prev, r_sim = rd.identity.cpu().numpy(), rd.prev.cpu().numpy(), rd.sim.cpu().numpy()
        report["track_reid"] = objects.reid_report(rd, tr.table, tr.extra, *reid)
        for row in report["tracks"]:
            t = row["track"] - 1
            row.update(identity=int(identity[t]), reid_prev=int(r_prev[t]), reid_sim=int(r_sim[t]))
        report["identities"] = objects.identity_rows(identity, r_prev, len(rows), [r["first"] for r in report["tracks"]],
                                                     [r["last"] for r in report["tracks"]], [r["length"] for r in rows])
    out_dir = args.mask_output_imgs
    write_json(f"{out_dir}/{name}", report)
    if not png:
        return
    rgb = (fl.rgb if fill else tr.rgb).cpu().numpy()
    for j, stem in enumerate(names):
        Image.fromarray(rgb[j]).save(f"{out_dir}/{stem}-tracks-mask.png")
    if reid:
        identity_rgb = identity_rgb.cpu().numpy()
        for j, stem in enumerate(names):
            Image.fromarray(identity_rgb[j]).save(f"{out_dir}/{stem}-identities-mask.png")
    if fill:
        on = (fl.labels > 0).cpu().numpy()
        for j, stem in enumerate(names):
            Image.fromarray(np.repeat((on[j] * np.uint8(255))[:, :, None], 3, axis=2)).save(f"{out_dir}/{stem}-filled-mask.png")
