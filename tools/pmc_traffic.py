"""Builds profiles/pmc_traffic.json from two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE; --kernel-trace only) of
`bench.py --full --no-cpu-baseline --steps 2098 --warmup 1049`: memory-side bytes of the resident step kernel per optimiser
step.  usage: pmc_traffic.py <dir with the FETCH_SIZE pass> <dir with the WRITE_SIZE pass> <out.json>"""
import csv, glob, json, sys

def per_launch(path, counter, pat="resident_train_kernel", min_frac=0.9):
    vals = []
    for f in glob.glob(path + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if pat in r["Kernel_Name"] and r["Counter_Name"] == counter:
                vals.append(float(r["Counter_Value"]))
    full = [v for v in vals if v >= min_frac * max(vals)]   # full-epoch launches only (1049 steps)
    return sum(full) / len(full), len(full)

fetch_kb, nf = per_launch(sys.argv[1], "FETCH_SIZE")
write_kb, nw = per_launch(sys.argv[2], "WRITE_SIZE")
steps = 1049
raw = (fetch_kb + write_kb) * 1024 / steps
corrected = (2 * fetch_kb + write_kb) * 1024 / steps
json.dump({
    "config": "bench.py (C2), resident_train_kernel<64,2,4,fast>, 1049 optimiser steps per launch",
    "FETCH_SIZE_KB_per_launch": round(fetch_kb, 1), "WRITE_SIZE_KB_per_launch": round(write_kb, 1),
    "launches_averaged": [nf, nw], "steps_per_launch": steps,
    "hbm_bytes_per_step_raw": int(raw), "hbm_bytes_per_step": int(corrected),
    "note": "separate rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) with --kernel-trace only; hbm_bytes_per_step doubles "
            "FETCH_SIZE as MI355X_MICROARCH.md prescribes for gfx950 wide reads (an upper bound here: most reads are "
            "8-byte granule polls and 4-byte state loads, whose width is uncalibrated); WRITE_SIZE is dominated by the "
            "mailbox granules (192 rows x 512 B per step)"}, open(sys.argv[3], "w"), indent=1)
print(open(sys.argv[3]).read())
