"""What the bench scripts of tools/ share: the timing of one callable and the writer of a note's marked block."""
import math
import re
import statistics


def time_ms(fn, warmup, groups, window_ms):
    """Device events around a window of calls of ``fn`` (at least ``window_ms`` long, sized from a calibration call) after
    ``warmup`` calls: the median, the least and the most of ``groups`` windows, in ms per call."""
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    steps = max(3, int(math.ceil(window_ms / max(e0.elapsed_time(e1), 1e-3))))
    out = []
    for _ in range(groups):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return {"ms": round(statistics.median(out), 4), "ms_min": round(min(out), 4), "ms_max": round(max(out), 4), "steps_per_window": steps}


def write_marked_block(path, text):
    """Replace what stands between ``<!-- device:begin -->`` and ``<!-- device:end -->`` of the note ``path`` by ``text``."""
    doc = open(path).read()
    doc, cnt = re.subn(r"(<!-- device:begin -->\n).*?(<!-- device:end -->)", lambda m: m.group(1) + text + m.group(2), doc, flags=re.S)
    assert cnt == 1, "the marked device block of the profile note"
    open(path, "w").write(doc)
