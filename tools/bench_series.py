"""Append a series of bench.py result lines of two builds, run alternately, to a timing file (development aid):
  bench_series.py out.txt parent_1.json change_1.json parent_2.json change_2.json ...
each file the one JSON line `python bench.py --gpus 1 --steps 20 --warmup 5` prints, the parent commit's build and this
change's taking turns in one session.  Writes the runs, both medians, the parent's spread (max - min) and whether this
change's median lies below the parent's by more than that spread."""
import json
import statistics
import sys

out, files = sys.argv[1], sys.argv[2:]
vals = [json.loads(open(f).read().strip().splitlines()[-1])["value"] for f in files]
parent, change = vals[0::2], vals[1::2]
mp, mc, spread = statistics.median(parent), statistics.median(change), max(parent) - min(parent)
lines = ["", "bench.py --gpus 1 --steps 20 --warmup 5, the parent commit and this change alternating, Mpixels/s of the lossless round trip:",
         "            run   parent       this change"]
lines += ["            %d     %.3f    %.3f" % (i + 1, p, c) for i, (p, c) in enumerate(zip(parent, change))]
lines += ["         median   %.3f    %.3f     parent's spread (max - min): %.3f" % (mp, mc, spread),
          "    condition: this change's median not below the parent's by more than the parent's spread: %s (%+.3f)" % ("met" if mc >= mp - spread else "NOT met", mc - mp)]
with open(out, "a") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
