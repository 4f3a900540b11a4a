"""The reports of ``-eval`` (handler.Handler.eval): the threshold, saliency and CRF-grid sweeps of eval_sweep.json, and
eval_objects.json, eval_match.json, eval_tracks.json, eval_boundary.json, eval_clean.json, eval_cut.json.  ``Stacks`` holds the stacks of one run on the device: each
is uploaded when a report first reads it, labelled (objects.label) once per source and matched (objects.match) once per source and
threshold list.  A report function takes (args, stacks) and returns (the dict of its file, its summary line); everything is scored on
the GPU and only counts come back.  ``write_json`` is the one writer of every report, here and in process.py."""
import json
import math
import os

import numpy as np
import torch

from . import boundary, clean, graphcut, metrics, objects, saliency, temporal

MATCH_MAX_OBJECTS = 64          # objects per frame and side that --match-iou matches and --track-iou follows
PREDICTIONS = ("mask", "crf", "cut")    # the stacks of the masker's own prediction: the soft mask, and its CRF / graph-cut refinement where the run has one


def _json_safe(obj):
    """NaN (an empty union or denominator) has no JSON spelling: it is written as null."""
    if isinstance(obj, dict):
        return {k: _json_safe(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_json_safe(v) for v in obj]
    return None if isinstance(obj, float) and math.isnan(obj) else obj


def write_json(path, obj, rank=0):
    """Rank 0 (data parallel: one writer) leaves `obj` at `path`, NaN as null, its directory made if need be."""
    if rank == 0:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as fp:
            json.dump(_json_safe(obj), fp, indent=1)


def fmt(v):
    return "nan" if v is None else f"{v:.6f}"


class Stacks:
    """The stacks of one -eval run by name, host arrays in `host`: "truth" (bool), "mask" (the probabilities, float32, read with the
    strict compare of --eval-thresh, main.py:964), the hard stacks "crf", "cut" (--graph-cut), "saliency", "saliency_crf" where the run has them, and the
    saliency sweep's inputs "sal" and "preds" (float32), and with --track-motion "frames" (uint8 [n,64,64,3]).  dev uploads a stack when it is first read; labelled and matched likewise.
    With --object-value the run also sets "frames" and `infer`, the critic as objects.value asks it (uint8 [b,64,64,3] -> [b])."""

    def __init__(self, args, device, **host):
        self.args, self.device, self.host, self._made = args, device, host, {}
        self.infer = None

    def _once(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    def names(self, among=("mask", "crf", "cut", "saliency", "saliency_crf")):
        """The hard stacks this run has, in the reports' order; among=PREDICTIONS: the ones the object reports describe."""
        return [name for name in among if name in self.host]

    def dev(self, name):
        dtype = np.float32 if name in ("mask", "sal", "preds") else None
        return self._once(name, lambda: torch.from_numpy(np.ascontiguousarray(self.host[name], dtype=dtype)).to(self.device))

    def thresh(self, name):
        return float(self.args.eval_thresh) if name == "mask" else None

    def cleaned(self, name):
        """--clean: clean.clean's result for "mask" (read at --eval-thresh, strict) or "crf", made once; its mask is the derived hard
        stack "mask_clean" / "crf_clean"."""
        return self._once(("clean", name), lambda: clean.clean(self.dev(name), thresh=self.thresh(name), **clean.spec_kwargs(self.args.clean)))

    def cut(self):
        """--graph-cut: graphcut.cut of the stack "mask" on the evaluation frames (the stack "frames", uint8), seeded with the strict
        compare of --eval-thresh; made once.  The run puts its mask into `host` as the hard stack "cut"."""
        return self._once(("cut",), lambda: graphcut.cut(self.dev("frames").contiguous(), self.dev("mask"), float(self.args.eval_thresh),
                                                         inclusive=False, **graphcut.spec_kwargs(self.args.graph_cut)))

    def object_source(self, name):
        """(stack, threshold) the object reports label for a source: with --clean the cleaned stack of a prediction (hard: None)."""
        if getattr(self.args, "clean", None) and name in PREDICTIONS:
            return self.cleaned(name).mask, None
        return self.dev(name), self.thresh(name)

    def labelled_all(self, name):
        """objects.label's result for a stack, labels and kept-pixel mask: a prediction with --connectivity and --min-area (the
        objects eval_objects.json counts), the truth unfiltered.  One call serves every report: labels, mask, found and kept do not
        depend on max_objects, and no report reads the table.  With --clean a prediction is labelled after the clean-up."""
        a = self.args
        src, thresh = self.object_source(name)
        return self._once(("label", name), lambda: objects.label(
            src, thresh=thresh, connectivity=a.connectivity, min_area=1 if name == "truth" else a.min_area,
            max_objects=MATCH_MAX_OBJECTS, want_labels=True, want_mask=name != "truth"))

    def labelled(self, name):
        """The objects the reports describe: labelled_all's, and with --object-value --min-value-drop, for a prediction, the ones
        that pass (selected)."""
        a = self.args
        if getattr(a, "object_value", False) and getattr(a, "min_value_drop", None) is not None and name != "truth":
            return self.selected(name)[0]
        return self.labelled_all(name)

    def valued(self, name):
        """--object-value: objects.value of a labelled prediction on the evaluation frames (the stack "frames", uint8), asked of
        self.infer, the critic in eval mode; made once."""
        a = self.args
        res = self.labelled_all(name)
        return self._once(("value", name), lambda: objects.value(
            self.infer, self.dev("frames").contiguous(), res.labels, res.kept, fill=a.object_value_fill, grow=a.object_value_grow,
            max_objects=MATCH_MAX_OBJECTS))

    def selected(self, name):
        """--min-value-drop: (the Objects that pass, objects.select's unscored, the keep table) of a prediction; made once."""
        def make():
            res = self.labelled_all(name)
            keep = objects.value_keep(self.valued(name).drop, res.kept, self.args.min_value_drop)
            return (*objects.select(res, keep), keep)
        return self._once(("select", name), make)

    def matched(self, name, iou, every=False):
        """objects.match of a labelled prediction against the labelled truth at the thresholds `iou`; every: of all its labelled
        objects, also when --min-value-drop selects among them."""
        pred = self.labelled_all(name) if every else self.labelled(name)
        return self._once(("match", name, tuple(iou), pred is self.labelled_all(name)), lambda: objects.match(
            pred.labels, self.labelled("truth").labels, iou=iou, max_objects=MATCH_MAX_OBJECTS))


def _head(args, **more):
    cleaned = {"clean": dict(args.clean)} if getattr(args, "clean", None) else {}
    return {"connectivity": args.connectivity, "min_area": args.min_area, "threshold": float(args.eval_thresh), **cleaned, **more}


def _blocks(st, report):
    """(prefix of the summary line, block) of every object source."""
    return [("" if name == "mask" else name + " ", report[name]) for name in st.names(PREDICTIONS)]


# ---------------------------------------------------------------------------------------------------------------- eval_sweep.json
def thresh_sweep(args, st):
    """--thresh-grid: the mask threshold only; the saliency threshold, which is also _saliency_post's normaliser, has a sweep of its
    own that renormalises per threshold (saliency_sweep)."""
    thr = metrics.parse_thresh_grid(args.thresh_grid)
    inter, union = metrics.iou_curve(st.dev("mask"), st.dev("truth"), thr)                              # strict >, main.py:964
    rep = metrics.curve_report(thr, inter.cpu().numpy(), union.cpu().numpy(), np.count_nonzero(st.host["truth"]))
    b = rep["best"]
    return rep, f"\nTHRESH SWEEP {len(thr)} thresholds, best {b['thresh']:.6g} (index {b['index']}) iou {b['iou']:.6f}"


def saliency_sweep(args, st):
    """--salience-grid: _saliency_post's hard mask at every threshold (float64), each with its own normaliser, scored against the truth
    on the GPU (saliency.sweep): the maps, the predictions and the truth are uploaded once and 2 T counts come back.  The global mode's
    mean is numpy's, of the host copy, so every row is what _saliency_post and get_iou's counts give at that threshold."""
    thr, glob, salM = saliency.parse_salience_grid(args.salience_grid), bool(args.salglobal), st.host["sal"]
    mean = np.where(salM >= 0, salM, 0.0).mean() if glob else None
    inter, union, _scale = saliency.sweep(st.dev("sal"), st.dev("preds"), st.dev("truth"), thr, glob, mean=mean)
    rep = saliency.sweep_report(thr, inter.cpu().numpy(), union.cpu().numpy(), np.count_nonzero(st.host["truth"]), salglobal=glob)
    rep = {"mode": "global" if glob else "frame", **rep}
    b = rep["best"]
    return rep, (f"\nSALIENCY SWEEP {len(rep['rows'])} thresholds ({rep['mode']}), best {b['thresh']:.6g} (index {b['index']}) "
                 f"iou {b['iou']:.6f}")


def crf_grid(args, st, tables):
    """--crf-grid: the tables Handler.crf left behind in this run, the mask's and then the saliency map's."""
    rep = dict(zip(("mask", "saliency"), tables))
    return rep, "\nCRF GRID " + "; ".join(f"{k}: {len(r['rows'])} points, best {r['best']['params']} iou {r['best']['iou']:.6f}"
                                          for k, r in rep.items())


# ---------------------------------------------------------------------------------------------------------------- the objects
def _objects_block(st, name):
    """One block of eval_objects.json: the kept pixels of a labelled stack and the unfiltered stack scored against the truth with
    metrics.iou_counts / iou_curve (with --clean both are the cleaned stack's).  Only the counts come back."""
    res, (src, thresh), truth = st.labelled_all(name), st.object_source(name), st.dev("truth")
    inter, union = metrics.iou_counts(res.mask, truth).tolist()
    if thresh is None:
        inter0, union0 = metrics.iou_counts(src, truth).tolist()
    else:
        inter0, union0 = (int(c[0]) for c in metrics.iou_curve(src, truth, [thresh]))
    kept, found = res.kept.cpu().numpy(), res.found.cpu().numpy()
    return {"inter": inter, "union": union, "iou": metrics.ratio(inter, union),
            "unfiltered": {"inter": inter0, "union": union0, "iou": metrics.ratio(inter0, union0)},
            "found": int(found.sum()), "kept": int(kept.sum()), "frames_without_objects": int(np.count_nonzero(kept == 0)),
            **_value_blocks(st, name)}


def _value_blocks(st, name):
    """--object-value: a source block's "value" (objects.value_report without the threshold) and, with --min-value-drop, "selected":
    the selected objects' count and their mask scored on the device with metrics.iou_counts."""
    a = st.args
    if not getattr(a, "object_value", False):
        return {}
    res, val, V = st.labelled_all(name), st.valued(name), a.min_value_drop
    if V is None:
        rep = objects.value_report(val, res.kept, a.object_value_fill, a.object_value_grow)
        rep.pop("min_value_drop")
        return {"value": rep}
    sel, unscored, keep = st.selected(name)
    rep = objects.value_report(val, res.kept, a.object_value_fill, a.object_value_grow, V, unscored=unscored)
    rep.pop("min_value_drop")
    inter, union = metrics.iou_counts(sel.mask, st.dev("truth")).tolist()
    return {"value": rep, "selected": {"kept": int(sel.kept.sum()), "inter": inter, "union": union, "iou": metrics.ratio(inter, union)}}


def objects_report(args, st):
    """-objects: the masks as objects, labelled, filtered and scored on the GPU.  With --object-value every block gains "value" (and
    with --min-value-drop "selected"), and the summary line the mean drop and the selected count."""
    report = _head(args)
    for name in st.names(PREDICTIONS):
        report[name] = _objects_block(st, name)
    report = _json_safe(report)

    def valued(b):
        if "value" not in b:
            return ""
        return f"; value drop mean {fmt(b['value']['drop']['mean'])}, selected {b['selected']['kept'] if 'selected' in b else b['value']['rows']}/{b['value']['rows']}"
    return report, f"\nOBJECTS conn={args.connectivity} min_area={args.min_area}: " + "; ".join(
        f"{pre}iou {fmt(b['iou'])} (unfiltered {fmt(b['unfiltered']['iou'])}), kept {b['kept']}/found {b['found']} objects{valued(b)}"
        for pre, b in _blocks(st, report))


def _match_values(st, name, iou):
    """--object-value with --match-iou: per threshold {"matched": {"n", "mean", "median"}, "spurious": {...}}, the value drops of the
    scored predicted objects (all of them, before any selection) whose best truth object reaches / does not reach that IoU -- Matches.best
    side 0, the compare the kernel makes, in integers; the statistics are host float64 (None for an empty side)."""
    res = st.labelled_all(name)
    best = st.matched(name, iou, every=True).best[:, 0].cpu().numpy().astype(np.int64)        # [n,K,4]: t, inter, area_p, area_t
    drop, kept = st.valued(name).drop.cpu().numpy().astype(np.float64), res.kept.cpu().numpy()
    scored = np.arange(drop.shape[1])[None] < np.clip(kept, 0, drop.shape[1])[:, None]
    inter, union = best[..., 1], best[..., 2] + best[..., 3] - best[..., 1]
    side = lambda d: {"n": int(d.size), "mean": float(d.mean()) if d.size else None, "median": float(np.median(d)) if d.size else None}
    out = []
    for m in objects.iou_milli(iou):
        reach = (inter > 0) & (1000 * inter >= m * union)
        out.append({"matched": side(drop[scored & reach]), "spurious": side(drop[scored & ~reach])})
    return out


def match_report(args, st):
    """--match-iou: those objects matched on the GPU to the truth's objects (objects.match).  Only the counts and the T sums of IoU
    come back.  With --object-value every threshold's entry gains "value" (_match_values)."""
    iou = objects.parse_match_iou(args.match_iou)
    report = _head(args, max_objects=MATCH_MAX_OBJECTS, iou=iou)
    for name in st.names(PREDICTIONS):
        m = st.matched(name, iou)
        report[name] = objects.match_report(m.pred_max, m.truth_max, m.matched_pred, m.matched_truth, objects.sum_iou(m.best, iou), iou,
                                            max_objects=MATCH_MAX_OBJECTS)
        if getattr(args, "object_value", False):
            for entry, v in zip(report[name]["per_iou"], _match_values(st, name, iou)):
                entry["value"] = v
    report = _json_safe(report)
    first = lambda b: b["per_iou"][0]
    return report, f"\nMATCH conn={args.connectivity} min_area={args.min_area} iou>={iou[0]:g} ({len(iou)} thresholds): " + "; ".join(
        f"{pre}matched {first(b)['matched_pred']}/{b['pred_objects']} predicted, {first(b)['matched_truth']}/"
        f"{b['truth_objects']} truth objects, f1 {fmt(first(b)['f1'])}, pq {fmt(first(b)['pq'])}" for pre, b in _blocks(st, report))


def _tracked(labelled, iou, gap=0, motion=None, reid=None):
    """(Tracks, one side of eval_tracks.json) of a labelled stack: tracked on the GPU, the length histogram and the link sums formed
    there; only the totals, 7 counts and 3 sums come back (with --track-gap also the links by gap and the missed frames).  motion:
    (bwd, search) of --track-motion; the side then gains "track_motion".  reid: (frames, similarity, window, area) of --track-reid;
    the tracks are chained into identities on the GPU (objects.appearance, objects.reid), the side gains "reid" (four counts) and the
    Reid comes back as the third item (None without it)."""
    K = MATCH_MAX_OBJECTS
    tr = objects.track(labelled.labels, iou=iou, max_objects=K, max_gap=gap, motion=motion[0] if motion else None)
    totals = torch.stack([tr.n_tracks, tr.n_links, tr.n_objects, tr.longest])
    more = {"max_gap": gap, "gap_links": tr.gap_links, "missed": tr.extra[:, 1].sum(dtype=torch.int64)} if gap else {}
    side = objects.track_report(totals, tr.table[:, 2], tr.table[:, 6].sum(dtype=torch.int64), tr.table[:, 7].sum(dtype=torch.int64),
                                (labelled.kept - K).clamp(min=0).sum(), **more)
    if motion:
        side["track_motion"] = objects.motion_report(*motion)
    rd = None
    if reid:
        rd = objects.reid(tr, objects.appearance(reid[0], labelled.labels, tr, max_objects=K), labelled.labels.shape[0], *reid[1:])
        counts = torch.stack([rd.n_eligible, rd.n_links, rd.n_identities, rd.longest]).tolist()
        side["reid"] = dict(zip(("eligible", "links", "identities", "longest"), (int(v) for v in counts)))
    return tr, side, rd


def _fill_block(labels, tracks, motion, truth):
    """--track-fill: one stack's "fill" of eval_tracks.json.  The frames its bridged links jump over are filled on the GPU (objects.fill)
    and the labelled pixels before and after are scored against the truth in one metrics.iou_counts launch; the four counts of the fill
    and the four of the score come back."""
    fl = objects.fill(labels, tracks, motion=motion[0] if motion else None, max_objects=MATCH_MAX_OBJECTS, want_table=False)
    (inter0, union0), (inter, union) = metrics.iou_counts(torch.stack([labels > 0, fl.labels > 0]), truth).tolist()
    return {**objects.fill_report(fl), "inter": inter, "union": union, "iou": metrics.ratio(inter, union),
            "inter_before": inter0, "union_before": union0, "iou_before": metrics.ratio(inter0, union0)}


def tracks_report(args, st):
    """--track-iou: the same objects followed from frame to frame on the GPU; with --match-iou the identity switches at its thresholds,
    from the matches eval_match.json reports.  --track-gap G tracks truth and predictions with the same G (objects.track's max_gap);
    the switches then follow the truth's adjacent links only, and every threshold's entry gains "fragments" (objects.fragments).
    --track-motion S tracks both along one field, temporal.flow of the evaluation frames as bytes (the stack "frames").
    --track-fill (with a gap) gives every predicted stack's side "fill" (_fill_block); the truth is tracked as ever and never filled.
    --track-reid S re-identifies truth and predictions with the same parameters on the stack "frames": every side gains "reid", and
    with --match-iou every threshold's entry "fragments_identity", objects.fragments on the identities of both sides."""
    t_iou = objects.parse_track_iou(args.track_iou)
    gap = int(getattr(args, "track_gap", 0) or 0)
    search = int(getattr(args, "track_motion", 0) or 0)
    motion = (temporal.flow(st.dev("frames"), search)[1], search) if search else None
    fill = bool(getattr(args, "track_fill", False) and gap)
    m_iou = objects.parse_match_iou(args.match_iou) if getattr(args, "match_iou", "") else None
    sim = getattr(args, "track_reid", None)
    reid = (st.dev("frames").contiguous(), sim, args.track_reid_window, args.track_reid_area) if sim else None
    truth_tr, truth_side, truth_rd = _tracked(st.labelled("truth"), t_iou, gap, motion, reid)
    report = _head(args, max_objects=MATCH_MAX_OBJECTS, track_iou=t_iou, truth=truth_side)
    truth_prev = torch.where(truth_tr.gap == 1, truth_tr.prev, 0) if gap else truth_tr.prev     # (without gaps every link has gap 1)
    for name in st.names(PREDICTIONS):
        pred_tr, side, pred_rd = _tracked(st.labelled(name), t_iou, gap, motion, reid)
        report[name] = {"pred": side}
        if fill:
            report[name]["fill"] = _fill_block(st.labelled(name).labels, pred_tr, motion, st.dev("truth"))
        if m_iou is not None:
            best = st.matched(name, m_iou).best
            counts = objects.switches(truth_prev, pred_tr.track, best, m_iou).cpu().numpy()
            report[name]["switches"] = [{"iou": t, "covered": int(c[0]), "continued": int(c[1]), "switches": int(c[2]),
                                         "switch_rate": int(c[2]) / int(c[1]) if c[1] else None} for t, c in zip(m_iou, counts)]
            if gap:
                for entry, v in zip(report[name]["switches"], objects.fragments(truth_tr.track, pred_tr.track, best, m_iou).cpu().numpy()):
                    entry["fragments"] = int(v)
            if reid:
                frag = objects.fragments(objects.identities(truth_tr.track, truth_rd.identity),
                                         objects.identities(pred_tr.track, pred_rd.identity), best, m_iou).cpu().numpy()
                for entry, v in zip(report[name]["switches"], frag):
                    entry["fragments_identity"] = int(v)
    report = _json_safe(report)
    p = report["mask"]["pred"]
    moved = f" motion<={search}" if search else ""
    again = f"; reid {p['reid']['links']} links, {p['reid']['identities']} identities" if reid else ""
    if gap:
        f = report["mask"].get("fill")
        filled = f"; filled {f['objects']} objects, iou {fmt(f['iou_before'])} -> {fmt(f['iou'])}" if f else ""
        return report, (f"\nTRACKS conn={args.connectivity} min_area={args.min_area} iou>={t_iou:g} gap<={gap}{moved}: {p['tracks']} tracks over "
                        f"{p['objects']} objects ({p['bridged_links']} of {p['links']} links bridged), mean length {fmt(p['mean_length'])}, "
                        f"longest {p['max_length']}; truth {truth_side['tracks']} tracks over {truth_side['objects']} objects{filled}{again}")
    return report, (f"\nTRACKS conn={args.connectivity} min_area={args.min_area} iou>={t_iou:g}{moved}: {p['tracks']} tracks over {p['objects']} "
                    f"objects, mean length {fmt(p['mean_length'])}, longest {p['max_length']}; truth {truth_side['tracks']} tracks over "
                    f"{truth_side['objects']} objects{again}")


# ---------------------------------------------------------------------------------------------------------------- the clean-up
def _scores(inter, union, pred_on, truth_on):
    return {"inter": inter, "union": union, "iou": metrics.ratio(inter, union), "precision": metrics.ratio(inter, pred_on),
            "recall": metrics.ratio(inter, truth_on)}


def clean_report(args, st):
    """--clean: every prediction cleaned on the GPU (clean.clean) and scored against the truth with metrics.iou_counts, beside the
    same figures of the uncleaned stack; the clean-up's own counts are summed.  Only counts come back."""
    truth = st.dev("truth")
    truth_on = int(np.count_nonzero(st.host["truth"]))
    report = {"clean": dict(args.clean), "threshold": float(args.eval_thresh)}
    for name in st.names(PREDICTIONS):
        res, src, thresh = st.cleaned(name), st.dev(name), st.thresh(name)
        sums = clean.clean_report(res.counts, args.clean)
        inter, union = metrics.iou_counts(res.mask, truth).tolist()
        if thresh is None:
            inter0, union0 = metrics.iou_counts(src, truth).tolist()
        else:
            inter0, union0 = (int(c[0]) for c in metrics.iou_curve(src, truth, [thresh]))
        report[name + "_clean"] = {**_scores(inter, union, sums["after_fill"], truth_on),
                                   "uncleaned": _scores(inter0, union0, sums["on"], truth_on),
                                   "counts": {k: sums[k] for k in clean.COUNTS}}
    report = _json_safe(report)
    return report, f"\nCLEAN {clean.spec_text(args.clean)}: " + "; ".join(
        f"{pre}iou {fmt(b['iou'])} (uncleaned {fmt(b['uncleaned']['iou'])}), {b['counts']['holes_filled']} holes filled, "
        f"{b['counts']['components_dropped']} components dropped"
        for pre, b in (("" if name == "mask" else name + " ", report[name + "_clean"]) for name in st.names(PREDICTIONS)))


# ---------------------------------------------------------------------------------------------------------------- the graph cut
def cut_report(args, st):
    """--graph-cut: the mask refined by graphcut.cut and scored against the truth on the device (metrics.iou_counts), beside the same
    counts of the plain threshold (metrics.iou_curve at --eval-thresh, the strict compare); the cut's own stats are summed.  Only
    counts come back."""
    res, truth = st.cut(), st.dev("truth")
    thresh = float(args.eval_thresh)
    sums = graphcut.cut_report(res.stats, args.graph_cut)
    lo, hi = graphcut.spec_band(args.graph_cut, thresh)
    inter, union = metrics.iou_counts(res.mask, truth).tolist()
    inter0, union0 = (int(c[0]) for c in metrics.iou_curve(st.dev("mask"), truth, [thresh]))
    truth_on = int(np.count_nonzero(st.host["truth"]))
    counts = lambda i, u, on: {"tp": i, "fp": on - i, "fn": truth_on - i, "inter": i, "union": u, "iou": metrics.ratio(i, u)}
    report = _json_safe({"graph_cut": dict(args.graph_cut), "threshold": thresh, "lo": lo, "hi": hi,
                         "before": counts(inter0, union0, sums["seed_on"]), "after": counts(inter, union, sums["on"]),
                         "stats": {k: v for k, v in sums.items() if k != "spec"}})
    return report, (f"\nCUT {graphcut.spec_text(args.graph_cut) or 'defaults'}: iou {fmt(report['after']['iou'])} (threshold alone "
                    f"{fmt(report['before']['iou'])}), {sums['changed']} cells changed, {sums['iterations']} cuts over {sums['frames']} frames, "
                    f"at most {sums['rounds']} rounds, {sums['not_converged']} not converged")


# ---------------------------------------------------------------------------------------------------------------- the outlines
def boundary_report(args, st):
    """--boundary-tol: the outline of every hard stack, and with -objects of the mask eval_objects.json scores (small objects removed),
    against the truth's outline on the GPU (boundary.score); only the per-frame counts come back."""
    tol = boundary.parse_boundary_tol(args.boundary_tol)
    stacks = [(name, st.dev(name), st.thresh(name)) for name in st.names()]
    if getattr(args, "clean", None):
        stacks += [(name + "_clean", st.cleaned(name).mask, None) for name in st.names(PREDICTIONS)]
    if getattr(args, "objects", False):
        stacks.append(("mask_objects", st.labelled("mask").mask, None))
    report = {"tol": tol, "tol2": boundary.tol_squared(tol), "threshold": float(args.eval_thresh)}
    for name, src, thr in stacks:
        b = boundary.score(src, st.dev("truth"), tol=tol, thresh=thr)
        report[name] = boundary.boundary_report(*(t.cpu().numpy() for t in b[:8]), tol)
    report = _json_safe(report)
    return report, f"\nBOUNDARY tol={tol[0]:g} ({len(tol)} tolerances): " + "; ".join(
        f"{name} f {fmt(report[name]['per_tol'][0]['f'])} boundary_iou {fmt(report[name]['per_tol'][0]['boundary_iou'])}"
        for name, _src, _thr in stacks)
