"""Folds `DVP_HOST_TIMING=1 apd ... --images-on host|gpu` logs (tools/images_timing.sh) into the figures of profiles/images_on_gpu.txt:
the whole schedule's wall time, the time to the first kernel (the [main] laps before the first view + that view's three
initialisation steps), the `[main] level N: images shared + resident on the device` laps, the per-view `images upload` lap per
pass, the passes' wall times and the device bytes the store holds.
usage: python3 tools/images_summary.py LOG [LOG ...]"""
import re, sys
def summarise(path):
    main_before_first, first_view, seen_view = 0.0, 0.0, False
    levels, uploads, passes, cur, real, dev_bytes, first_done = [], {}, {}, None, None, None, False
    for ln in open(path, errors="replace"):
        m = re.match(r"\[main\] (.*): ([0-9.]+) ms", ln)
        if m:
            if not seen_view:
                main_before_first += float(m.group(2))
            lm = re.match(r"level (\d+): images shared", m.group(1))
            if lm:
                levels.append((int(lm.group(1)), float(m.group(2))))
            pm = re.match(r"pass (\d+): helpers started", m.group(1))
            if pm:
                cur = int(pm.group(1))
            continue
        if ln.startswith("Processing image:") and "done" not in ln:
            seen_view = True
        m = re.match(r"\s+\[host\] (InuputInitialization|SupportInitialization|CudaSpaceInitialization)[^:]*: ([0-9.]+) ms", ln)
        if m and not first_done:
            first_view += float(m.group(2))
            if m.group(1).startswith("Cuda"):
                first_done = True
        m = re.match(r"\s+\[host\]   \. images upload: ([0-9.]+) ms", ln)
        if m:
            uploads.setdefault(cur, []).append(float(m.group(1)))
        m = re.match(r"Pass (\d+): (\d+) views in ([0-9.]+) ms", ln)
        if m:
            passes[int(m.group(1))] = float(m.group(3))
        m = re.match(r"\[main\] decoded images on the device: (\d+) bytes", ln)
        if m:
            dev_bytes = int(m.group(1))
        m = re.match(r"real\s+(\d+)m([0-9.]+)s", ln)
        if m:
            real = 60 * int(m.group(1)) + float(m.group(2))
    return dict(real=real, first_kernel=main_before_first + first_view, levels=levels, uploads=uploads, passes=passes, dev_bytes=dev_bytes)
for p in sys.argv[1:]:
    s = summarise(p)
    print(p)
    print("  whole schedule: %.2f s; to the first kernel (main laps + first view's three init steps): %.1f ms" % (s["real"] or -1, s["first_kernel"]))
    print("  level laps (images shared + resident): " + ", ".join("L%d %.1f ms" % l for l in s["levels"]))
    print("  per-view 'images upload' lap, mean [min .. max] ms per pass: " + "; ".join("p%s %.2f [%.2f .. %.2f]" % (k, sum(v) / len(v), min(v), max(v)) for k, v in sorted(s["uploads"].items(), key=lambda kv: -1 if kv[0] is None else kv[0])))
    print("  pass wall ms: " + ", ".join("p%d %.0f" % kv for kv in sorted(s["passes"].items())))
    if s["dev_bytes"] is not None:
        print("  decoded images on the device: %d bytes" % s["dev_bytes"])
