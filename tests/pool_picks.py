"""The kernels' 2x2 max-pool picks, decoded for the oracle (oracle/hourglass_ref.critic_apply(picks=...)), and the strict check that every
pick is the right one.

Why: some pooled windows have their two largest candidates within ~1e-6 relative of each other; fp32 and float64 can order those
differently, and dy then goes to a neighbouring pixel -- a discrete change of every weight gradient at and below that layer that no
rounding tolerance covers.  The float64 oracle therefore FOLLOWS the kernels' picks, and ``check_picks`` separately asserts that a pick
differs from float64's only on such near-ties (and never on an exact tie, where max_pool2d's first index is the rule), so that
following them cannot hide a tie-rule or indexing bug of the pooling itself.

Pick = position in the window, row-major: 0 = (0,0), 1 = (0,1), 2 = (1,0), 3 = (1,1).  Two device formats:
  nibbles  the fused chfak-1 path (cgs_amd.hourglass.critic_forward, engine.HourglassEngine.cbuf["am{i}"]): int32 [n, hp, wp, co/8],
           channel c in word c // 8, bits 4 (c % 8) .. +3; 0xF = dead (no positive value in the window).
  bytes    the shape-generic path (cgs_amd.generic, generic_engine.GenericEngine.cbuf["am{i}"]): uint8 [n, hp, wp, co]; >= 4 = dead.
Decoders return (pick int64 [n, co, hp, wp] with dead windows mapped to 0, dead bool [n, co, hp, wp]).

Both engines keep the critic's passes of a phase-2 step in slot order [B | A | rep | inj]; the oracle takes them as [A, B, rep, inj]."""
import torch
import torch.nn.functional as F

from oracle import hourglass_ref as orc

KEYS = orc.ENC_CONV_KEYS
NEAR_TIE = 2e-6           # relative gap of a window's two largest float64 values up to which fp32 may pick either
GATE = 1e-4               # |max| (relative to the conv output's maximum) above which the ReLU gate must agree with float64
TIE = 1e-12               # an exact tie as float64 sees it: the CPU's float64 convolution of identical patches can differ in the last
                          # bits from one pixel position to the next (measured: 5.5e-17 absolute on flat frames), fp32 rounding is 1e-7


def decode_nibbles(am):
    am = am.detach().cpu().to(torch.int64) & 0xFFFFFFFF          # int32 words -> their unsigned bit patterns
    n, hp, wp, words = am.shape
    shifts = 4 * torch.arange(8, dtype=torch.int64)
    code = (am.unsqueeze(-1) >> shifts) & 0xF                     # [n, hp, wp, words, 8]
    code = code.reshape(n, hp, wp, 8 * words).permute(0, 3, 1, 2).contiguous()
    dead = code == 0xF
    return code.masked_fill(dead, 0), dead


def decode_bytes(am):
    code = am.detach().cpu().to(torch.int64).permute(0, 3, 1, 2).contiguous()
    dead = code >= 4
    return code.masked_fill(dead, 0), dead


def decode(am):
    return decode_nibbles(am) if am.dtype == torch.int32 else decode_bytes(am)


def buffer_picks(buf, n_slots):
    """Decoded picks of all four stages of a critic buffer dict (am0..am3, first n_slots images): ([pick per stage], [dead per stage])."""
    out = [decode(buf[f"am{i}"][:n_slots]) for i in range(4)]
    return [p for p, _ in out], [d for _, d in out]


def oracle_order(per_stage, n):
    """Per-stage tensors over the slots [B | A | rep | inj] (the first 2 n + n_mix of them) -> one list of four stage tensors per
    critic pass, in the oracle's order [A, B, rep, inj] (phase2_loss's ``picks``)."""
    slots = per_stage[0].shape[0] // n
    where = {"B": 0, "A": 1, "rep": 2, "inj": 3}
    return [[t[where[k] * n:(where[k] + 1) * n] for t in per_stage] for k in ("A", "B", "rep", "inj") if where[k] < slots]


def _windows(y):
    N, C, H, W = y.shape
    return y.reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)


def check_picks(pc, inputs, picks, dead, chunk=64, what=""):
    """For each pooling stage: the float64 convolution of that stage's device-computed input (``inputs[i]``: NHWC, fp32 or uint8
    frames, device or host, images aligned with ``picks[i]``), and asserts
      - the ReLU gate (dead or not) agrees with float64 wherever the window's |max| > GATE of the conv output's maximum;
      - the pick is max_pool2d's FIRST index wherever the window's two largest values are exactly equal (to TIE: float64's own noise);
      - the pick is the argmax wherever those two values are more than NEAR_TIE relative apart.
    Returns per stage (cells where a live pick differs from float64's argmax, the largest relative gap among them).  Callers bound
    the count: a few near-ties per million cells are rounding; more is a bug that pinning the oracle would otherwise follow."""
    out = []
    for i, key in enumerate(KEYS):
        x_all, pk_all, dd_all = inputs[i], picks[i], dead[i]
        w, b = pc[key + ".weight"].double(), pc[key + ".bias"].double()
        gmax, gate_worst, count, gap_worst = 0.0, 0.0, 0, 0.0
        for a in range(0, x_all.shape[0], chunk):
            x = x_all[a:a + chunk].detach().cpu()
            x = x.double() / 255.0 if x.dtype == torch.uint8 else x.double()
            y = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1)      # pre-ReLU: max(relu) = relu(max)
            cells = _windows(y)
            top2 = cells.topk(2, dim=-1).values
            top, second = top2[..., 0], top2[..., 1]
            tied = top - second <= TIE * top.abs()
            first = (cells >= (top - TIE * top.abs()).unsqueeze(-1)).to(torch.uint8).argmax(-1)     # the first maximum: max_pool2d's rule
            pk, dd = pk_all[a:a + chunk], dd_all[a:a + chunk]
            live = ~dd
            gmax = max(gmax, float(y.abs().max()))
            gate_bad = (live & (top <= 0)) | (dd & (top > 0))
            if gate_bad.any():
                gate_worst = max(gate_worst, float(top[gate_bad].abs().max()))
            gap = (top - second) / top.abs().clamp_min(1e-300)
            chk = live & (top > 0)
            tie_bad = chk & tied & (pk != first)
            assert not tie_bad.any(), f"{what} {key}: {int(tie_bad.sum())} exactly tied windows whose pick is not max_pool2d's first index"
            mism = chk & (pk != first)
            clear_bad = mism & (gap > NEAR_TIE)
            assert not clear_bad.any(), (f"{what} {key}: {int(clear_bad.sum())} picks differ from float64's argmax on windows whose two "
                                         f"largest values are up to {float(gap[clear_bad].max()):.2e} relative apart (> {NEAR_TIE})")
            count += int(mism.sum())
            if mism.any():
                gap_worst = max(gap_worst, float(gap[mism].max()))
        assert gate_worst <= GATE * gmax, f"{what} {key}: ReLU gate differs from float64 at a window of |max| {gate_worst:.3e} (conv max {gmax:.3e})"
        out.append((count, gap_worst))
    return out


def report(flips, what):
    """One printed line per test: the flip count and largest gap of every stage."""
    txt = ", ".join(f"{k} {c} (gap {g:.1e})" if c else f"{k} 0" for k, (c, g) in zip(KEYS, flips))
    print(f"pool-pick flips vs float64, {what}: {txt}")
    return sum(c for c, _ in flips)
