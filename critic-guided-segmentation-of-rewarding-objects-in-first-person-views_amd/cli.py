"""Command line of the reference's ``main.py`` (flags at main.py:1463-1533, dispatch at :1535-1570):

    python main.py -train --model DIR
    python main.py -process [-concatenated] [--binarymaskthreshold t] --model DIR --source-imgs S --mask-output-imgs R
    python main.py -process -fit [--fit-spatial s] [--fit-range r] ...      (this build's own: frames of any one size, 64..4096 a side)
    python main.py -process --source-video IN.mp4 --overlay-video OUT.mp4 [--smooth R] ...      (this build's own: a video in, masks
                                                            smoothed along time, a GPU-composed overlay video out)
    python main.py -test --model DIR --output-video V       (evaluation sweep + the evaluation video V/iou=....mp4)
    python main.py -train -critic '' -masker '' -vismasker --model DIR      (DIR/curves.mp4, -pred-sorted.mp4, -GT-sorted.mp4)

Every flag of the reference parses (same names, defaults and the ``type=bool`` quirk: ``-cload False`` is
still True, as in the reference); flags whose code path is outside this build raise NotImplementedError
when reached instead of being silently ignored.  ``-grabcut`` is the one flag the reference itself declares and never reads (main.py:1485):
it is parsed and does nothing here too; the refinement it names is this build's ``--graph-cut SPEC`` (graphcut.py)."""
import argparse


def build_parser():
    p = argparse.ArgumentParser()
    for flag in ("-train", "-cleaned", "-frozen", "-clippify", "-debug", "-noinject", "-freeze", "-viscritic",
                 "-vismasker", "-visdataset", "-trunk", "-higheval", "-separate", "-salience", "-process_salience",
                 "-grabcut", "-crf", "-directeval", "-soft", "-resimages", "-noevalmode", "-eval", "-process", "-test",
                 "-concatenated", "-softmask"):
        p.add_argument(flag, action="store_true")
    # (this build's own switch, not a flag of the reference) -process / -eval with fp16 activations and weights, fp32 accumulation
    p.add_argument("-fp16", action="store_true")
    # (this build's own flags) -eval sweeps, scored on the GPU (metrics.py): --thresh-grid "0.01-0.05-0.5" or "lo:hi:n" scores the masks
    # at every threshold (the grid main.py:974 left commented out); --crf-grid "w1=5,22;it=2,10" makes -crf the parameter grid search
    # main.py:1226-1263 is written as.  Both leave {model}/eval_sweep.json
    p.add_argument("--thresh-grid", type=str, default="")
    p.add_argument("--crf-grid", type=str, default="")
    # (this build's own flag) -eval -salience --salience-grid "0.25-0.5-0.75" or "lo:hi:n": the saliency baseline thresholded at every
    # value, each with its own normaliser (--salience-thresh is both), scored on the GPU (saliency.py); adds "saliency" to eval_sweep.json
    p.add_argument("--salience-grid", type=str, default="")
    # (this build's own flags) -objects: the masks of -process / -eval labelled into connected components on the GPU (objects.py),
    # components below --min-area pixels removed.  -process leaves objects.json and {stem}-objects-mask.png, -eval eval_objects.json.
    # The two options default to 1 and 8 (filled in by check_objects_flags, which has to see whether they were given)
    p.add_argument("-objects", action="store_true")
    p.add_argument("--min-area", type=int, default=None)
    p.add_argument("--connectivity", type=int, default=None)
    # (this build's own flag) -eval -objects --match-iou "0.5-0.75-0.95" or "lo:hi:n": the predicted objects matched to the objects of
    # the labelled truth at these IoU thresholds on the GPU (objects.match); leaves {model}/eval_match.json
    p.add_argument("--match-iou", type=str, default="")
    # (this build's own flag) -objects --track-iou T with -process or -eval: the objects followed from frame to frame on the GPU
    # (objects.track); leaves {model}/eval_tracks.json, or {R}/tracks.json and {R}/{stem}-tracks-mask.png
    p.add_argument("--track-iou", type=str, default="")
    # (this build's own flag) --track-iou T --track-gap G: an object may be missing for up to G frames (0..8, default 0) and keeps its
    # track (objects.track's max_gap); check_objects_flags turns it into an int
    p.add_argument("--track-gap", type=str, default=None)
    # (this build's own flag) --track-iou T --track-motion S: the earlier frame's labels are carried along block vectors of the 64 x 64
    # frames, up to S cells a frame (0..4, default 0 = off), before they are compared (objects.track's motion); an int after the check
    p.add_argument("--track-motion", type=str, default=None)
    # (this build's own flag) --track-iou T --track-gap G --track-fill: the frames a bridged link jumps over get the mask of the link's
    # tail object, carried there along the vectors of --track-motion (objects.fill); -process leaves {stem}-filled-mask.png and paints
    # {stem}-tracks-mask.png from the filled labels, -eval adds "fill" to eval_tracks.json.  Not for --source-video
    p.add_argument("--track-fill", action="store_true")
    # (this build's own flag) --track-iou T --track-reid S: tracks that do not overlap in time, lie at most --track-reid-window W frames
    # apart (1..1024, default 64) and whose 64-bin colour histograms intersect to at least S (in (0, 1]) are chained into one identity
    # on the GPU (objects.appearance, objects.reid); --track-reid-area A (default 64) is the pixels a track needs over its life.
    # -process leaves {stem}-identities-mask.png and adds to tracks.json, -eval adds to eval_tracks.json.  Not for --source-video
    p.add_argument("--track-reid", type=str, default=None)
    p.add_argument("--track-reid-window", type=str, default=None)
    p.add_argument("--track-reid-area", type=str, default=None)
    # (this build's own flags) -objects --object-value: the critic is asked about every object (objects.value): the frame is rebuilt on
    # the GPU once per object with that object replaced -- by the frame of smallest value (--object-value-fill low, the training rule's
    # B, the default), by the frame's mean background colour (mean) or by a colour R,G,B -- together with the cells within
    # --object-value-grow cells of it (0..4, default 0), and the object's value is how far the critic's value of the frame falls.
    # --min-value-drop V keeps the objects whose drop is at least V and renumbers them (objects.select): the mask PNGs, --track-iou,
    # --match-iou and everything on top then describe those.  -process adds to objects.json / tracks.json and leaves
    # {stem}-valued-mask.png, -eval adds to eval_objects.json / eval_match.json.  Not for --source-video, not with -noevalmode
    p.add_argument("--object-value", action="store_true")
    p.add_argument("--object-value-fill", type=str, default=None)
    p.add_argument("--object-value-grow", type=str, default=None)
    p.add_argument("--min-value-drop", type=str, default=None)
    # (this build's own flag) -eval --boundary-tol "0-1-2-3" or "lo:hi:n": every evaluated stack's outline against the truth's outline at
    # these tolerances in pixels -- boundary F, boundary IoU and the Hausdorff distance -- on the GPU (boundary.score); leaves
    # {model}/eval_boundary.json
    p.add_argument("--boundary-tol", type=str, default="")
    # (this build's own flags) -process -fit: frames of any one size from 64 to 4096 pixels a side, shrunk to the network's 64 x 64 grid
    # on the GPU and the masks brought back to the frame's size by joint bilateral upsampling along the frame's edges (fit.py).
    # --fit-spatial (cells) and --fit-range (colour units of 0..255) default to 1 and 16, filled in by check_fit_flags
    p.add_argument("-fit", action="store_true")
    p.add_argument("--fit-spatial", type=float, default=None)
    p.add_argument("--fit-range", type=float, default=None)
    # (this build's own flags) -process --source-video IN --overlay-video OUT: the frames of a video file (decoded by ffmpeg) instead of a
    # folder of stills, through the -fit machinery, and the masks drawn on the frames at the frames' size as a video (overlay.py).
    # --smooth R filters the masks along time over +-R frames first (temporal.py; 0 = off), --smooth-range is its colour sigma,
    # --smooth-motion S lets its taps follow block-matched motion of up to S cells a frame (0 = off).  The defaults (0, 16, 0, overlay,
    # 0,255,0, 0.5, 1) are filled in by check_video_flags, which has to see what was given.
    # --overlay-tracks T labels the thresholded masks (8-connected, components below --overlay-min-area A cells dropped), follows the
    # objects through the stream at link IoU T (objects.TrackStream) and draws every object in its track's colour with its bounding box,
    # --overlay-boxes B pixels thick (0: none), and its track number (overlay.compose_tracks); leaves {R}/{stem}-objects.json and
    # {R}/{stem}-tracks.json.  A and B default to 1.  --overlay-gap G (0..8, default 0) is --track-gap for this stream: an object that
    # has no mask for up to G frames comes back under its number and colour.  --overlay-motion S (0..4, default 0) is --track-motion for
    # this stream: the labels are carried along block vectors of the shrunk frames before they are compared.  --overlay-fill (with
    # --overlay-gap G >= 1) is --track-fill for this stream: the frames a bridged link jumps over get the tail's mask, drawn hatched
    # (objects.FillStream, overlay.compose_tracks(age=)); the overlay then runs G frames behind the masks
    p.add_argument("--source-video", type=str, default="")
    p.add_argument("--overlay-video", type=str, default="")
    p.add_argument("--smooth", type=int, default=None)
    p.add_argument("--smooth-range", type=float, default=None)
    p.add_argument("--smooth-motion", type=int, default=None)
    p.add_argument("--overlay-layout", type=str, default=None)
    p.add_argument("--overlay-color", type=str, default=None)
    p.add_argument("--overlay-alpha", type=float, default=None)
    p.add_argument("--overlay-outline", type=int, default=None)
    p.add_argument("--overlay-tracks", type=str, default=None)
    p.add_argument("--overlay-min-area", type=int, default=None)
    p.add_argument("--overlay-boxes", type=int, default=None)
    p.add_argument("--overlay-gap", type=str, default=None)
    p.add_argument("--overlay-motion", type=str, default=None)
    p.add_argument("--overlay-fill", action="store_true")
    # (this build's own flags) --clean SPEC with -process or -eval, --overlay-clean SPEC with --source-video: the thresholded mask (with
    # -crf the CRF mask) cleaned on the GPU before anything reads it (clean.py): "hyst=0.8;open=1;close=2;fill=16;shape=cross;conn=4" --
    # hysteresis with the strong threshold, opening and closing radii 0..4, holes of up to so many pixels filled, square | cross, 4 | 8.
    # -process leaves {stem}-clean-mask.png and clean.json, -eval eval_clean.json; -objects, --match-iou, --track-iou and
    # --boundary-tol then describe the cleaned masks, and the overlay video draws them.  check_clean_flags parses both into dicts
    p.add_argument("--clean", type=str, default=None)
    p.add_argument("--overlay-clean", type=str, default=None)
    # (this build's own flag) --graph-cut SPEC with -process or -eval: the mask refined by an exact min cut on the GPU (graphcut.py), GrabCut
    # without the mixtures: "lo=0.1;hi=0.9;lambda=50;it=3;bins=8;conn=8", every key optional ("" is the defaults) -- cells below lo are
    # hard background, cells above hi hard foreground (defaults: half way from the threshold to 0 and to 1), the rest is decided by up
    # to `it` cuts with colour histograms of `bins` bins a channel as the models and `lambda` times a contrast weight between `conn`
    # neighbours.  The cut mask takes the place the CRF mask takes (so not with -crf): -process leaves {stem}-cut-mask.png and cut.json,
    # -eval eval_cut.json; --clean, -objects, --match-iou, --track-iou and --boundary-tol then describe the cut masks.  The
    # reference's -grabcut stays what it is there, parsed and never read.  check_cut_flags parses the spec into a dict
    p.add_argument("--graph-cut", type=str, default=None)
    for flag in ("-masker", "-critic", "-cload", "-mload", "-staticnorm", "-visbesteval", "-salglobal"):
        p.add_argument(flag, type=bool, default=True)
    p.add_argument("--salience-thresh", type=float, default="1.5")
    p.add_argument("--eval-thresh", type=float, default=0.05)
    p.add_argument("--dropout", type=float, default=0.3)
    p.add_argument("--lr", type=float, default=0.00005)   # parsed, never read (as in the reference)
    p.add_argument("--threshrew", type=float, default=0)
    p.add_argument("--trainasvis", type=int, default=0)
    p.add_argument("--false", type=bool, default=False)
    p.add_argument("--envname", type=str, default="Treechop")
    p.add_argument("--visname", type=str, default="curves")
    p.add_argument("--datamode", type=str, default="trunk")
    p.add_argument("--purevis", type=str, default="")
    p.add_argument("--sortidx", type=int, default=1)
    p.add_argument("--chfak", type=int, default=1)
    p.add_argument("--shift", type=int, default=12)
    p.add_argument("--lfak", type=int, default=5)
    p.add_argument("--neck", type=int, default=32)
    p.add_argument("--clossfak", type=int, default=5)
    p.add_argument("--cepochs", type=int, default=15)
    p.add_argument("--mepochs", type=int, default=1)
    p.add_argument("--high-rew-thresh", type=float, default=0.7)
    p.add_argument("--low-rew-thresh", type=float, default=0.3)
    p.add_argument("--L2", type=float, default=0.0)
    p.add_argument("--L1", type=float, default=0.5)
    p.add_argument("--saveevery", type=int, default=5)
    p.add_argument("--visevery", type=int, default=100)
    p.add_argument("--rewidx", type=int, default=1)
    p.add_argument("--gammas", type=str, default="0.98-0.97-0.96-0.95")
    p.add_argument("--testsize", type=int, default=5000)
    p.add_argument("--datasize", type=int, default=100000)
    p.add_argument("--name", type=str, default="default-model")
    p.add_argument("--model", type=str, default="default-model")
    p.add_argument("--runs", type=int, default=1)
    p.add_argument("--source-imgs", type=str, default="")
    p.add_argument("--mask-output-imgs", type=str, default="results")
    p.add_argument("--output-video", type=str, default="")
    p.add_argument("--binarymaskthreshold", type=float, default=0.5)
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    args.workers = (1, 1, 1)
    args.live = not args.frozen
    args.inject = not args.noinject
    args.name = args.model
    if args.test:
        args.eval = True
        args.train = True if not args.cload else False
        args.visbesteval = True
        args.crf = False
        args.salience = True
    check_sweep_flags(args)
    check_objects_flags(args)
    check_video_flags(args)
    check_fit_flags(args)
    check_clean_flags(args)
    check_cut_flags(args)
    return args


def check_sweep_flags(args):
    """--thresh-grid / --crf-grid / --salience-grid: malformed grids and combinations that could not run are refused here, before any GPU work."""
    if args.thresh_grid:
        from .metrics import parse_thresh_grid
        parse_thresh_grid(args.thresh_grid)
        if not args.eval:
            raise ValueError("--thresh-grid sweeps the threshold of -eval: give -eval (or -test)")
    if args.crf_grid:
        from .crf import parse_crf_grid
        parse_crf_grid(args.crf_grid)
        if args.process:
            raise ValueError("--crf-grid scores every point against the labels of -eval; -process has none")
        if not (args.crf and args.eval):
            raise ValueError("--crf-grid is the parameter grid of -eval -crf: give both (-test switches -crf off)")
    if args.salience_grid:
        from .saliency import frame_k, parse_salience_grid, PIXELS
        thr = parse_salience_grid(args.salience_grid)
        if args.process:
            raise ValueError("--salience-grid scores every threshold against the labels of -eval; -process has none")
        if not (args.eval and args.salience):
            raise ValueError("--salience-grid sweeps the saliency baseline of -eval -salience: give both (or -test)")
        if not args.salglobal and (frame_k(thr) > PIXELS - 1).any():
            raise ValueError(f"--salience-grid {args.salience_grid!r}: with -salglobal '' a threshold t picks each map's int({PIXELS} * t)-th "
                             "smallest value: every t must be below 1")


def check_objects_flags(args):
    """-objects / --min-area / --connectivity / --match-iou / --track-iou / --track-gap / --track-motion / --track-fill / --boundary-tol:
    combinations that could not run and a malformed --match-iou, --track-iou, --track-gap, --track-motion or --boundary-tol are refused
    here, before any GPU work; the defaults (--min-area 1, --connectivity 8, --track-gap 0 and --track-motion 0 as ints) are filled in.
    --boundary-tol needs -eval, not -objects; --track-fill needs --track-iou and a --track-gap of at least 1, and no --source-video.
    --track-reid S needs --track-iou and no --source-video; it becomes a float, and --track-reid-window / --track-reid-area (which need
    it) become ints, 64 and 64 by default.  --object-value needs -objects, no --source-video and no -noevalmode; --object-value-fill
    (low | mean | R,G,B, default low), --object-value-grow (0..4, default 0) and --min-value-drop (a finite number, default none) need
    it and are parsed here.  The two defaults are judgements, not tuned values."""
    given = [f for f, v in (("--min-area", args.min_area), ("--connectivity", args.connectivity)) if v is not None]
    if args.match_iou:
        from .objects import parse_match_iou
        given.append("--match-iou")
        parse_match_iou(args.match_iou)
        if args.process:
            raise ValueError("--match-iou matches the objects against the labels of -eval; -process has none")
        if args.objects and not args.eval:
            raise ValueError("--match-iou belongs to -eval -objects: give -eval (or -test)")
    if args.boundary_tol:
        from .boundary import parse_boundary_tol
        parse_boundary_tol(args.boundary_tol)
        if not args.eval:
            raise ValueError("--boundary-tol scores the outlines against the labels of -eval: give -eval (or -test)")
    if args.track_iou:
        from .objects import parse_track_iou
        given.append("--track-iou")
        parse_track_iou(args.track_iou)
    if args.track_gap is not None:
        from .objects import parse_track_gap
        if not args.track_iou:
            raise ValueError("--track-gap belongs to --track-iou: give --track-iou T")
        args.track_gap = parse_track_gap(args.track_gap)
    else:
        args.track_gap = 0
    if args.track_motion is not None:
        from .objects import parse_track_motion
        if not args.track_iou:
            raise ValueError("--track-motion belongs to --track-iou: give --track-iou T")
        args.track_motion = parse_track_motion(args.track_motion)
    else:
        args.track_motion = 0
    if args.track_fill:
        if not args.track_iou:
            raise ValueError("--track-fill belongs to --track-iou: give --track-iou T --track-gap G")
        if not args.track_gap:
            raise ValueError("--track-fill fills the frames that a bridged link jumps over: give --track-gap G with G in 1..8")
        if args.source_video:
            raise ValueError("--track-fill with --source-video: outside this build (the stream would have to look --overlay-gap frames "
                             "ahead before it draws a frame); the video path's own flag is --overlay-fill, which does")
    reid_more = [f for f, v in (("--track-reid-window", args.track_reid_window), ("--track-reid-area", args.track_reid_area)) if v is not None]
    if args.track_reid is None:
        if reid_more:
            raise ValueError(f"{' / '.join(reid_more)} belong to --track-reid: give --track-reid S")
    else:
        from . import objects as _objects
        if not args.track_iou:
            raise ValueError("--track-reid belongs to --track-iou: give --track-iou T")
        if args.source_video:
            raise ValueError("--track-reid with --source-video: outside this build (the stream path has no identity layer)")
        args.track_reid = _objects.parse_track_reid(args.track_reid)
        args.track_reid_window = (_objects.REID_WINDOW if args.track_reid_window is None
                                  else _objects.parse_track_reid_window(args.track_reid_window))
        args.track_reid_area = _objects.REID_MIN_AREA if args.track_reid_area is None else _objects.parse_track_reid_area(args.track_reid_area)
    value_more = [f for f, v in (("--object-value-fill", args.object_value_fill), ("--object-value-grow", args.object_value_grow),
                                 ("--min-value-drop", args.min_value_drop)) if v is not None]
    if not args.object_value:
        if value_more:
            raise ValueError(f"{' / '.join(value_more)} belong to --object-value: give --object-value")
    else:
        from . import objects as _objects
        given.append("--object-value")
        if args.source_video:
            raise ValueError("--object-value with --source-video: outside this build (the stream path does not score its objects)")
        if args.noevalmode:
            raise ValueError("--object-value with -noevalmode: Dropout would make the values noise; the critic is asked in eval mode")
        args.object_value_fill = (_objects.VALUE_FILL if args.object_value_fill is None
                                  else _objects.parse_object_value_fill(args.object_value_fill))
        args.object_value_grow = _objects.VALUE_GROW if args.object_value_grow is None else _objects.parse_object_value_grow(args.object_value_grow)
        args.min_value_drop = None if args.min_value_drop is None else _objects.parse_min_value_drop(args.min_value_drop)
    if not args.objects:
        if given:
            raise ValueError(f"{' / '.join(given)} belong to -objects: give -objects")
    elif not (args.process or args.eval):
        raise ValueError("-objects labels the masks of -process or -eval (or -test): give one of them")
    args.min_area = 1 if args.min_area is None else args.min_area
    args.connectivity = 8 if args.connectivity is None else args.connectivity
    if args.min_area < 1:
        raise ValueError(f"--min-area {args.min_area}: an object has at least 1 pixel")
    if args.connectivity not in (4, 8):
        raise ValueError(f"--connectivity {args.connectivity}: 4 or 8")
    if args.objects and args.process and not args.binarymaskthreshold and not args.crf:
        raise ValueError("-process -objects labels the thresholded mask (or with -crf the CRF mask): --binarymaskthreshold 0 without "
                         "-crf leaves no binary mask")


def check_fit_flags(args):
    """-fit / --fit-spatial / --fit-range: combinations that could not run and sigmas outside the filter's range are refused here, before
    any GPU work; the defaults (--fit-spatial 1, --fit-range 16) are filled in."""
    given = [f for f, v in (("--fit-spatial", args.fit_spatial), ("--fit-range", args.fit_range)) if v is not None]
    if not args.fit:
        if given:
            raise ValueError(f"{' / '.join(given)} belong to -fit: give -fit")
        return
    if not args.process:
        raise ValueError("-fit resizes the frames of -process: give -process")
    if args.eval:
        raise ValueError("-fit is for -process; the data of -eval and -test is 64 x 64 .npy")
    if args.salience or args.process_salience:
        raise ValueError("-fit with -salience / -process_salience: upsampled saliency maps are outside this build")
    from .fit import SIGMA_RANGE, SIGMA_SPATIAL, check_sigmas
    args.fit_spatial, args.fit_range = check_sigmas(SIGMA_SPATIAL if args.fit_spatial is None else args.fit_spatial,
                                                    SIGMA_RANGE if args.fit_range is None else args.fit_range,
                                                    names=("--fit-spatial", "--fit-range"))


def check_video_flags(args):
    """--source-video / --overlay-video and the --smooth* / --overlay-* options: combinations that could not run and values out of range
    are refused here, before any GPU work; the defaults (--smooth 0, --smooth-range 16, --smooth-motion 0, --overlay-layout overlay,
    --overlay-color 0,255,0, --overlay-alpha 0.5, --overlay-outline 1; with --overlay-tracks T also --overlay-min-area 1, --overlay-boxes 1, --overlay-gap 0, --overlay-motion 0) are filled
    in (--overlay-fill needs --source-video, --overlay-tracks and an --overlay-gap of at least 1), --overlay-color becomes (r, g, b), args.overlay_alpha256 is round(256 alpha), --overlay-tracks becomes a float (None without the
    flag), and -fit is switched on: a video goes through the -fit machinery.  The frame size is checked after the probe
    (check_video_size)."""
    given = [f for f, v in (("--overlay-video", args.overlay_video or None), ("--smooth", args.smooth), ("--smooth-range", args.smooth_range),
                            ("--smooth-motion", args.smooth_motion),
                            ("--overlay-layout", args.overlay_layout), ("--overlay-color", args.overlay_color),
                            ("--overlay-alpha", args.overlay_alpha), ("--overlay-outline", args.overlay_outline),
                            ("--overlay-tracks", args.overlay_tracks), ("--overlay-min-area", args.overlay_min_area),
                            ("--overlay-boxes", args.overlay_boxes), ("--overlay-gap", args.overlay_gap),
                            ("--overlay-motion", args.overlay_motion),
                            ("--overlay-fill", True if getattr(args, "overlay_fill", False) else None)) if v is not None]
    if not args.source_video:
        if given:
            raise ValueError(f"{' / '.join(given)} belong to --source-video: give --source-video")
        return
    if not args.process:
        raise ValueError("--source-video is the source of -process: give -process")
    if not args.overlay_video:
        raise ValueError("--source-video writes its masks as an overlay video: give --overlay-video")
    for on, what in ((args.eval, "-eval / -test"), (args.crf, "-crf"), (args.objects, "-objects"),
                     (args.salience or args.process_salience, "-salience / -process_salience"), (args.concatenated, "-concatenated")):
        if on:
            raise ValueError(f"--source-video with {what}: outside this build (a video source gives the masks and the overlay video only)")
    from . import overlay, parallel, temporal
    from .fit import check_sigmas
    if parallel.env_world()[2] > 1:
        raise ValueError(f"--source-video with {parallel.env_world()[2]} ranks: a video is one stream, run one process")
    args.smooth = temporal.check_radius(0 if args.smooth is None else args.smooth, least=0, name="--smooth")
    _, args.smooth_range = check_sigmas(1.0, temporal.SIGMA_RANGE if args.smooth_range is None else args.smooth_range,
                                        names=("", "--smooth-range"))
    args.smooth_motion = temporal.check_search(0 if args.smooth_motion is None else args.smooth_motion, least=0, name="--smooth-motion")
    if args.smooth_motion and not args.smooth:
        raise ValueError("--smooth-motion steers the taps of --smooth: give --smooth R")
    def named(flag, fn, value):
        try:
            return fn(value)
        except ValueError as e:
            raise ValueError(f"{flag}: {e}") from None
    args.overlay_layout = overlay.LAYOUT if args.overlay_layout is None else args.overlay_layout
    args.overlay_panels = named("--overlay-layout", overlay.panels, args.overlay_layout)
    args.overlay_color = named("--overlay-color", overlay.parse_color, overlay.COLOR if args.overlay_color is None else args.overlay_color)
    args.overlay_alpha = overlay.ALPHA if args.overlay_alpha is None else args.overlay_alpha
    args.overlay_alpha256 = named("--overlay-alpha", overlay.to_alpha256, args.overlay_alpha)
    args.overlay_outline = named("--overlay-outline", overlay.check_outline,
                                 overlay.OUTLINE if args.overlay_outline is None else args.overlay_outline)
    if args.overlay_tracks is None:
        extra = [f for f, v in (("--overlay-min-area", args.overlay_min_area), ("--overlay-boxes", args.overlay_boxes),
                                ("--overlay-gap", args.overlay_gap), ("--overlay-motion", args.overlay_motion),
                                ("--overlay-fill", True if getattr(args, "overlay_fill", False) else None)) if v is not None]
        if extra:
            raise ValueError(f"{' / '.join(extra)} belong to --overlay-tracks: give --overlay-tracks T")
    else:
        from .objects import parse_track_iou
        try:
            args.overlay_tracks = parse_track_iou(args.overlay_tracks)
        except ValueError as e:
            raise ValueError(f"--overlay-tracks: {str(e).replace('--track-iou ', '', 1)}") from None
        if not args.binarymaskthreshold:
            raise ValueError("--overlay-tracks labels the thresholded mask: --binarymaskthreshold 0 leaves none")
        args.overlay_min_area = 1 if args.overlay_min_area is None else args.overlay_min_area
        if args.overlay_min_area < 1:
            raise ValueError(f"--overlay-min-area {args.overlay_min_area}: an object has at least 1 cell")
        args.overlay_boxes = named("--overlay-boxes", overlay.check_boxes, overlay.BOXES if args.overlay_boxes is None else args.overlay_boxes)
        from .objects import parse_track_gap
        args.overlay_gap = 0 if args.overlay_gap is None else parse_track_gap(args.overlay_gap, "--overlay-gap")
        from .objects import parse_track_motion
        args.overlay_motion = 0 if args.overlay_motion is None else parse_track_motion(args.overlay_motion, "--overlay-motion")
        if getattr(args, "overlay_fill", False) and not args.overlay_gap:
            raise ValueError("--overlay-fill fills the frames that a bridged link jumps over: give --overlay-gap G with G in 1..8")
    args.fit = True


def check_clean_flags(args):
    """--clean / --overlay-clean: a malformed spec and combinations that could not run are refused here, before any GPU work; both
    become clean.parse_clean's dict (None without the flag).  `hyst` needs a soft source (no -crf) and must not lie below the
    threshold the path compares with: --binarymaskthreshold for -process and --source-video, --eval-thresh for -eval."""
    from .clean import parse_clean
    if args.overlay_clean is not None:
        if not args.source_video:
            raise ValueError("--overlay-clean cleans the masks of --source-video: give --source-video (the flag of -process and -eval "
                             "is --clean)")
        args.overlay_clean = spec = parse_clean(args.overlay_clean, "--overlay-clean")
        if not args.binarymaskthreshold:
            raise ValueError("--overlay-clean cleans the thresholded mask: --binarymaskthreshold 0 leaves nothing to clean")
        if spec["hyst"] is not None and spec["hyst"] < args.binarymaskthreshold:
            raise ValueError(f"--overlay-clean hyst={spec['hyst']!r} lies below --binarymaskthreshold {args.binarymaskthreshold!r}: the "
                             "strong threshold is the higher of the two")
    if args.clean is None:
        return
    if args.source_video:
        raise ValueError("--clean with --source-video: the flag there is --overlay-clean")
    if not (args.process or args.eval):
        raise ValueError("--clean cleans the masks of -process or -eval (or -test): give one of them")
    args.clean = spec = parse_clean(args.clean, "--clean")
    if args.process and not args.binarymaskthreshold and not args.crf:
        raise ValueError("-process --clean cleans the thresholded mask (or with -crf the CRF mask): --binarymaskthreshold 0 without "
                         "-crf leaves nothing to clean")
    if spec["hyst"] is None:
        return
    if args.crf:
        raise ValueError("--clean hyst=... with -crf: the CRF mask is hard, it has no strong pixels (hysteresis needs the soft mask)")
    for on, flag, thr in ((args.process, "--binarymaskthreshold", args.binarymaskthreshold), (args.eval, "--eval-thresh", args.eval_thresh)):
        if on and spec["hyst"] < thr:
            raise ValueError(f"--clean hyst={spec['hyst']!r} lies below {flag} {thr!r}: the strong threshold is the higher of the two")


def check_cut_flags(args):
    """--graph-cut: a malformed or out-of-range spec and combinations that could not run are refused here, before any GPU work; the
    flag becomes graphcut.parse_spec's dict (None without the flag).  The cut is seeded at the threshold its path compares with --
    --binarymaskthreshold for -process, --eval-thresh for -eval -- and lo <= threshold <= hi must hold for each (lo and hi default to
    graphcut.default_band of that threshold).  Not with --source-video (the stream path has no refinement slot) and not with -crf: two
    refinements, one slot for the refined mask."""
    if args.graph_cut is None:
        return
    from .graphcut import parse_spec, spec_band
    if args.source_video:
        raise ValueError("--graph-cut with --source-video: outside this build (a video source gives the masks and the overlay video only)")
    if not (args.process or args.eval):
        raise ValueError("--graph-cut refines the masks of -process or -eval (or -test): give one of them")
    if args.crf:
        raise ValueError("--graph-cut with -crf: two refinements and one slot for the refined mask; give one of them")
    args.graph_cut = spec = parse_spec(args.graph_cut, "--graph-cut")
    if isinstance(getattr(args, "clean", None), dict) and args.clean["hyst"] is not None:
        raise ValueError("--clean hyst=... with --graph-cut: the cut mask is hard, it has no strong pixels (hysteresis needs the soft mask)")
    for on, flag, thr in ((args.process, "--binarymaskthreshold", args.binarymaskthreshold), (args.eval, "--eval-thresh", args.eval_thresh)):
        if on:
            try:
                spec_band(spec, thr)
            except ValueError as e:
                raise ValueError(f"{e} ({flag} {thr!r})") from None


def check_video_size(w, h, panels):
    """The probed frame size of --source-video: 64..4096 a side (fit.check_size), and an even height and an even width of the finished
    frame, which yuv420p needs.  Called after the probe and before the first frame is decoded."""
    from .fit import check_size
    try:
        check_size(h, w)
    except ValueError as e:
        raise ValueError(f"--source-video: {e}") from None
    if h % 2 or (panels * w) % 2:
        raise ValueError(f"--source-video: frames of {w}x{h} give a video of {panels * w}x{h}; yuv420p needs an even width and height "
                         "(odd sizes are outside this build)")


def main(argv=None):
    from . import vis
    from .handler import Handler
    args = parse_args(argv)
    if (args.viscritic or args.vismasker) and not args.trainasvis:
        vis.refuse_unbuilt(args)            # before any GPU work
    if args.source_video:
        from . import video_in
        video_in.find_ffmpeg(), video_in.find_ffprobe()     # FileNotFoundError before any GPU work
    H = Handler(args)
    if args.train:
        H.load_data()
    if args.trainasvis:
        raise NotImplementedError("--trainasvis (dataset visualisation) is outside this build's scope")
    if args.cload:
        H.load_models(modelnames=[H.criticname])
    if args.mload:
        H.load_models(modelnames=[H.maskername])
    if args.train:
        if args.critic:
            H.critic_pipe(mode="train")
            H.save_models(modelnames=[H.criticname])
        if args.masker:
            H.segmentation_training()
            H.save_models(modelnames=[H.maskername])
    if args.eval:
        H.eval()
    if args.viscritic or args.vismasker:
        H.visualize()
    if args.process:
        H.segment(folder=args.source_imgs)
    return H
