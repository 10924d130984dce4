"""A fixed table of ILLEGAL calls of the WPE entry points of libadn.so, one line each: `entry point | case | return code | message`.

Every call is refused by the argument checks, before the first HIP call, so no device is needed and no pointer is followed (the
buffers are host memory of the right size).  A change that must not move a return code, the order of the checks or a byte of a
message (a refactoring of the WPE sections of csrc/adn_api.hip) is checked by comparing two runs as text:

    ADN_LIBADN_PATH=.../libadn_parent.so python tools/wpe_refusals.py > before.txt      # built as tools/spectral_digest.py says
    python tools/wpe_refusals.py > after.txt ; diff before.txt after.txt

Every case is one change to a legal call: each null pointer, each size at 0, each parameter field just outside its range and
NaN, params = NULL with a state one byte too small (which pins the default taps: 20 for the single-channel functions,
32 / channels for the joint ones, channels = 1 included; the offline functions need no workspace, so there the default shows as
"channels * taps <= 32" at 32 / channels + 1 taps only through explicit params), misalignment, overlap, col0 + n_frames > width,
more rows than slots, lookahead != 0, n_streams % channels, the forget rule at (2, 16), and for the pool of recordings
(adn_wpe_mc_stream_pool) n_slots % channels, n_rows % channels and the three rules of a group's rows.  A call that is NOT refused would reach
the device: the script stops there with an error instead of printing a line."""
import ctypes
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from audiodenoiser_amd import _lib  # noqa: E402

L = _lib.load()
NAN = math.nan
N, T, F = 2, 6, 5                                       # rows (or groups), frames, bins of the offline and online calls
PLAN = dict(n_fft=64, hop=16, window=16, block=4, lookahead=0)
MEM = ctypes.create_string_buffer(1 << 22)              # one host buffer: addresses only, 64-byte aligned from `BASE`
BASE = (ctypes.addressof(MEM) + 63) & ~63
SPEC, OUT, MAG, STATE, SSTATE, Y = (BASE + i * (1 << 19) for i in range(6))


def size_of(fn, *args):
    need = ctypes.c_size_t(0)
    rc = fn(*args, ctypes.byref(need))
    assert rc == 0, (fn.__name__, args, L.adn_last_error())
    return need.value


def params(cls, defaults, **kw):
    return cls(*[kw.get(k, v) for k, v in defaults])


OFFLINE = (("taps", 4), ("delay", 3), ("iterations", 3), ("loading", 1e-3), ("power_floor", 1e-3))
STREAM = (("taps", 4), ("delay", 3), ("forget", 0.99), ("loading", 300.0), ("power_floor", 0.01), ("smooth", 0.9))
OFFLINE_BAD = (("taps", 0), ("taps", 33), ("delay", 0), ("delay", 9), ("iterations", 0), ("iterations", 9), ("loading", 0.9e-6),
               ("loading", 1.0001), ("loading", NAN), ("power_floor", 0.0), ("power_floor", 1.0001), ("power_floor", NAN))
STREAM_BAD = (("taps", 0), ("taps", 33), ("delay", 0), ("delay", 9), ("forget", 0.9499), ("forget", 1.0001), ("forget", NAN),
              ("loading", 0.9999), ("loading", 1.0001e6), ("loading", NAN), ("power_floor", 0.0), ("power_floor", 1.0001),
              ("power_floor", NAN), ("smooth", -1e-3), ("smooth", 1.0), ("smooth", NAN))


def refuse(name, case, order, args):
    """One line for the call ``name(*[args[k] for k in order])``, which must be refused."""
    fn = getattr(L, name)
    vals = [args[k] for k in order]
    vals = [ctypes.byref(v) if isinstance(v, ctypes.Structure) else v for v in vals]
    rc = fn(*vals)
    if rc == 0:
        raise SystemExit(f"{name} | {case}: NOT refused -- the table must hold illegal calls only")
    print(f"{name} | {case} | {rc} | {L.adn_last_error().decode()}", flush=True)


def table(name, order, good, cases):
    for case, change in cases:
        refuse(name, case, order, {**good, **change})


def param_cases(cls, defaults, bad, channels):
    cases = [(f"{k}={v}", dict(params=params(cls, defaults, **{k: v}))) for k, v in bad]
    if channels is not None:
        cases += [(f"channels={c}", dict(channels=c)) for c in (0, 9)]
        cases += [("channels*taps=33", dict(channels=3, params=params(cls, defaults, taps=11))),
                  ("default taps + 1", dict(params=params(cls, defaults, taps=32 // channels + 1)))]
    return cases


def offline(mc):
    pre = "adn_wpe_mc" if mc else "adn_wpe"
    lead = ["n", "channels"] if mc else ["n"]
    for channels in ((1, 2, 3, 8) if mc else (None,)):
        p = params(_lib.WpeParamsStruct, OFFLINE)
        good = dict(spec=SPEC, n=N, channels=channels, t=T, f=F, params=p, ws=None, ws_bytes=0, out=OUT, mag=MAG, width=T, stream=None,
                    bytes=ctypes.byref(ctypes.c_size_t(0)))
        tag = f"C={channels} " if mc else ""
        sizes = [(f"{tag}{k}=0", {k: 0}) for k in ("n", "t", "f")]
        pc = [(tag + c, ch) for c, ch in param_cases(_lib.WpeParamsStruct, OFFLINE, OFFLINE_BAD, channels)]
        big = [(f"{tag}grid too large", dict(n=(1 << 31) // (channels or 1) - 1, f=1 << 20, params=params(_lib.WpeParamsStruct, OFFLINE, taps=1)))]
        if mc and channels >= 2:
            big.append((f"{tag}n_groups*channels=2^31", dict(n=(1 << 31) // channels + 1)))
        table(pre + "_workspace_bytes", lead + ["t", "f", "params", "bytes"], good, [(tag + "bytes=NULL", dict(bytes=None))] + sizes + pc + big)
        table(pre, ["spec"] + lead + ["t", "f", "params", "ws", "ws_bytes", "out", "mag", "width", "stream"], good,
              [(tag + "spec=NULL", dict(spec=None)), (tag + "spec_out=NULL", dict(out=None))] + sizes + pc + big +
              [(tag + "width<n_frames", dict(width=T - 1)), (tag + "spec misaligned", dict(spec=SPEC + 4)),
               (tag + "spec_out misaligned", dict(out=OUT + 4)), (tag + "mag_out misaligned", dict(mag=MAG + 2)),
               (tag + "overlap", dict(out=SPEC + 8)), (tag + "in place", dict(out=SPEC))])


def online(mc):
    pre = "adn_wpe_mc" if mc else "adn_wpe"
    cls = _lib.WpeStreamParamsStruct
    for channels in ((1, 2, 3, 8) if mc else (None,)):
        c = channels or 1
        lead = (["n", "channels"] if mc else ["n"])
        sizer = getattr(L, pre + "_stream_state_bytes")
        p = params(cls, STREAM, taps=2 if c == 8 else 4)
        tag = f"C={channels} " if mc else ""

        def need(slots, f, pp):
            return size_of(sizer, *((slots, channels, f) if mc else (slots, f)), ctypes.byref(pp) if pp is not None else None)
        # the default taps, pinned by the size of the state that params = NULL asks for: 20, or 32 / channels
        taps0 = 32 // channels if mc else 20
        assert need(N, F, None) == need(N, F, params(cls, STREAM, taps=taps0)) != need(N, F, params(cls, STREAM, taps=taps0 - 1))
        good = dict(spec=SPEC, n=N, channels=channels, t=T, f=F, first=0, params=p, state=STATE, state_bytes=need(N, F, p), slots=N,
                    out=OUT, mag=MAG, width=T, col0=0, stream=None, bytes=ctypes.byref(ctypes.c_size_t(0)))
        pc = [(tag + k, ch) for k, ch in param_cases(cls, STREAM, STREAM_BAD, channels)]
        if mc and channels >= 2:
            pc.append((tag + "forget rule", dict(params=params(cls, STREAM, taps=32 // channels, forget=0.98))))
        if mc and channels == 2:
            pc.append((tag + "forget rule at (2, 16): 0.984 < 1 - 1/64", dict(params=params(cls, STREAM, taps=16, forget=0.984))))
        table(pre + "_stream_state_bytes", ["slots"] + (["channels"] if mc else []) + ["f", "params", "bytes"], good,
              [(tag + "bytes=NULL", dict(bytes=None)), (tag + "n_slots=0", dict(slots=0)), (tag + "n_slots=2^20+1", dict(slots=(1 << 20) + 1)),
               (tag + "n_bins=0", dict(f=0)), (tag + "n_bins=2^20+1", dict(f=(1 << 20) + 1))] + pc)
        table(pre + "_online", ["spec"] + lead + ["t", "f", "first", "params", "state", "state_bytes", "slots", "out", "mag", "width", "col0",
                                                   "stream"], good,
              [(tag + "spec=NULL", dict(spec=None)), (tag + "spec_out=NULL", dict(out=None))] +
              [(f"{tag}{k}=0", {k: 0}) for k in ("n", "t", "f")] +
              [(tag + "first_frame=-1", dict(first=-1)), (tag + "first_frame+n_frames=2^31", dict(first=(1 << 31) - T))] + pc +
              [(tag + "state=NULL", dict(state=None)), (tag + "n_slots=0", dict(slots=0)),
               (tag + "state one byte short", dict(state_bytes=good["state_bytes"] - 1)),
               (tag + "params=NULL, state one byte short of the default taps", dict(params=None, state_bytes=need(N, F, None) - 1)),
               (tag + "state misaligned", dict(state=STATE + 4)), (tag + "more rows than slots", dict(n=N + 1, state_bytes=need(N + 1, F, p))),
               (tag + "col0=-1", dict(col0=-1)), (tag + "width=0", dict(width=0)), (tag + "col0+n_frames>width", dict(col0=1)),
               (tag + "spec misaligned", dict(spec=SPEC + 4)), (tag + "spec_out misaligned", dict(out=OUT + 4)),
               (tag + "mag_out misaligned", dict(mag=MAG + 2)), (tag + "overlap", dict(out=SPEC + 8)), (tag + "in place", dict(out=SPEC))])
        # the lockstep stream: n_streams = 2 channels streams, so that a joint call has two groups
        ns = 2 * c
        fb = PLAN["n_fft"] // 2 + 1
        plan = dict(PLAN, max_steps=4)
        sbytes = size_of(L.adn_stream_state_bytes, ns, *plan.values())
        assert sbytes <= 1 << 19 and need(ns // c, fb, p) <= 1 << 19
        good = dict(sstate=SSTATE, sbytes=sbytes, y=Y, ns=ns, channels=channels, first=0, steps=1, final=-1, **plan, params=p, state=STATE,
                    state_bytes=need(ns // c, fb, p), stream=None)
        cases = ([(tag + "state=NULL", dict(sstate=None)), (tag + "n_streams=0", dict(ns=0)), (tag + "n_fft=48", dict(n_fft=48)),
                  (tag + "hop=0", dict(hop=0)), (tag + "window=15", dict(window=15)), (tag + "block=0", dict(block=0)),
                  (tag + "max_steps=0", dict(max_steps=0)), (tag + "stream state one byte short", dict(sbytes=sbytes - 1)),
                  (tag + "stream state misaligned", dict(sstate=SSTATE + 4)), (tag + "lookahead=1", dict(lookahead=1)),
                  (tag + "y=NULL", dict(y=None)), (tag + "y misaligned", dict(y=Y + 2)), (tag + "first_step=-1", dict(first=-1)),
                  (tag + "n_steps=0", dict(steps=0)), (tag + "n_steps>max_steps", dict(steps=5)), (tag + "final_length=0", dict(final=0))] + pc +
                 [(tag + "WPE state=NULL", dict(state=None)), (tag + "WPE state one byte short", dict(state_bytes=good["state_bytes"] - 1)),
                  (tag + "params=NULL, WPE state one byte short of the default taps", dict(params=None, state_bytes=need(ns // c, fb, None) - 1)),
                  (tag + "WPE state misaligned", dict(state=STATE + 4))])
        if mc and channels >= 2:
            cases.append((tag + "n_streams % channels", dict(ns=ns + 1, sbytes=size_of(L.adn_stream_state_bytes, ns + 1, *plan.values()))))
        table(pre + "_stream", ["sstate", "sbytes", "y", "ns"] + (["channels"] if mc else []) + ["first", "steps", "final", *plan, "params",
                                                                                                 "state", "state_bytes", "stream"], good, cases)


def pool():
    cls = _lib.WpeStreamParamsStruct
    p = params(cls, STREAM)
    slots, ring, fb = 3, 4096, PLAN["n_fft"] // 2 + 1
    pbytes = size_of(L.adn_stream_pool_state_bytes, slots, *PLAN.values(), ring)
    assert pbytes <= 1 << 19

    def need(pp):
        return size_of(L.adn_wpe_stream_state_bytes, slots, fb, ctypes.byref(pp) if pp is not None else None)

    def rows(*r):
        return (_lib.StreamPoolRow * len(r))(*[_lib.StreamPoolRow(*x) for x in r])
    good = dict(pstate=SSTATE, pbytes=pbytes, slots=slots, **PLAN, ring=ring, rows=rows((0, 0, -1), (2, 1, -1)), n_rows=2, y=Y, params=p,
                state=STATE, state_bytes=need(p), stream=None)
    table("adn_wpe_stream_pool", ["pstate", "pbytes", "slots", *PLAN, "ring", "rows", "n_rows", "y", "params", "state", "state_bytes", "stream"],
          good,
          [("state=NULL", dict(pstate=None)), ("n_slots=0", dict(slots=0)), ("n_fft=48", dict(n_fft=48)), ("ring_samples=1", dict(ring=1)),
           ("pool state one byte short", dict(pbytes=pbytes - 1)), ("pool state misaligned", dict(pstate=SSTATE + 4)),
           ("lookahead=1", dict(lookahead=1)), ("y=NULL", dict(y=None)), ("y misaligned", dict(y=Y + 2)), ("rows=NULL", dict(rows=None)),
           ("n_rows=0", dict(n_rows=0)), ("n_rows=257", dict(n_rows=257)), ("slot outside", dict(rows=rows((0, 0, -1), (3, 1, -1)))),
           ("slot twice", dict(rows=rows((1, 0, -1), (1, 1, -1)))), ("step=-1", dict(rows=rows((0, -1, -1), (2, 1, -1)))),
           ("final_length=0", dict(rows=rows((0, 0, 0), (2, 1, -1))))] +
          param_cases(cls, STREAM, STREAM_BAD, None) +
          [("WPE state=NULL", dict(state=None)), ("WPE state one byte short", dict(state_bytes=need(p) - 1)),
           ("params=NULL, WPE state one byte short of the default taps", dict(params=None, state_bytes=need(None) - 1)),
           ("WPE state misaligned", dict(state=STATE + 4))])


def pool_mc():
    """adn_wpe_mc_stream_pool: what the pool call refuses, what the joint parameters refuse, and the rules of a recording's rows."""
    cls = _lib.WpeStreamParamsStruct
    ring, fb = 4096, PLAN["n_fft"] // 2 + 1

    def rows(*r):
        return (_lib.StreamPoolRow * len(r))(*[_lib.StreamPoolRow(*x) for x in r])
    for channels in (1, 2, 3, 8):
        slots = 3 * channels                                             # three recordings
        p = params(cls, STREAM, taps=2 if channels == 8 else 4)
        tag = f"C={channels} "
        pbytes = size_of(L.adn_stream_pool_state_bytes, slots, *PLAN.values(), ring)
        assert pbytes <= 1 << 19

        def need(pp, n=3):
            return size_of(L.adn_wpe_mc_stream_state_bytes, n, channels, fb, ctypes.byref(pp) if pp is not None else None)

        def table_of(*recordings):                                       # (recording, step, final_length) -> its C rows
            return rows(*[(r * channels + c, k, final) for r, k, final in recordings for c in range(channels)])
        good = dict(pstate=SSTATE, pbytes=pbytes, slots=slots, channels=channels, **PLAN, ring=ring, rows=table_of((2, 1, -1), (0, 0, -1)),
                    n_rows=2 * channels, y=Y, params=p, state=STATE, state_bytes=need(p), stream=None)
        cases = ([(tag + "state=NULL", dict(pstate=None)), (tag + "n_slots=0", dict(slots=0)), (tag + "n_fft=48", dict(n_fft=48)),
                  (tag + "ring_samples=1", dict(ring=1)), (tag + "pool state one byte short", dict(pbytes=pbytes - 1)),
                  (tag + "pool state misaligned", dict(pstate=SSTATE + 4)), (tag + "lookahead=1", dict(lookahead=1)),
                  (tag + "y=NULL", dict(y=None)), (tag + "y misaligned", dict(y=Y + 2)), (tag + "rows=NULL", dict(rows=None)),
                  (tag + "n_rows=0", dict(n_rows=0)), (tag + "n_rows=257", dict(n_rows=257)),
                  (tag + "slot outside", dict(rows=table_of((3, 1, -1), (0, 0, -1)))),
                  (tag + "slot twice", dict(rows=table_of((1, 0, -1), (1, 0, -1)))),
                  (tag + "step=-1", dict(rows=table_of((2, -1, -1), (0, 0, -1)))),
                  (tag + "final_length=0", dict(rows=table_of((2, 1, 0), (0, 0, -1))))] +
                 [(tag + k, ch) for k, ch in param_cases(cls, STREAM, STREAM_BAD, channels)] +
                 [(tag + "WPE state=NULL", dict(state=None)), (tag + "WPE state one byte short", dict(state_bytes=need(p) - 1)),
                  (tag + "params=NULL, WPE state one byte short of the default taps", dict(params=None, state_bytes=need(None) - 1)),
                  (tag + "WPE state misaligned", dict(state=STATE + 4))])
        if channels >= 2:
            swapped = [(2 * channels + c, 1, -1) for c in range(channels)]
            swapped[0], swapped[1] = swapped[1], swapped[0]
            shifted = [(1 + c, 0, -1) for c in range(channels)]
            other_step = [(c, 0 if c else 1, -1) for c in range(channels)]
            other_final = [(c, 0, -1 if c else 40) for c in range(channels)]
            cases += [(tag + "forget rule", dict(params=params(cls, STREAM, taps=32 // channels, forget=0.98))),
                      (tag + "n_slots % channels", dict(slots=slots + 1, pbytes=size_of(L.adn_stream_pool_state_bytes, slots + 1, *PLAN.values(), ring))),
                      (tag + "n_rows % channels", dict(n_rows=2 * channels - 1)),
                      (tag + "first slot no multiple of channels", dict(rows=rows(*shifted), n_rows=channels)),
                      (tag + "slots not in channel order", dict(rows=rows(*swapped), n_rows=channels)),
                      (tag + "rows differ in step", dict(rows=rows(*other_step), n_rows=channels)),
                      (tag + "rows differ in final_length", dict(rows=rows(*other_final), n_rows=channels))]
        table("adn_wpe_mc_stream_pool", ["pstate", "pbytes", "slots", "channels", *PLAN, "ring", "rows", "n_rows", "y", "params", "state",
                                         "state_bytes", "stream"], good, cases)


def main():
    for mc in (False, True):
        offline(mc)
    for mc in (False, True):
        online(mc)
    pool()
    pool_mc()


if __name__ == "__main__":
    main()
