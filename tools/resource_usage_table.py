"""tools/resource_usage_table.py LABEL=LOG [LABEL=LOG ...] — one line per kernel and build from hipcc's -Rpass-analysis=kernel-resource-usage remarks
(python lvi-exc_amd/build.py --force --verbose 2> LOG): VGPRs, AGPRs, scratch bytes per lane, static LDS bytes and waves per SIMD.  With several logs the kernels
whose figures differ between the first build and any other are marked."""
import re
import subprocess
import sys


def parse(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: +Function Name: (\S+)", line)
        if m:
            name = m.group(1); out[name] = {}
            continue
        m = re.search(r"remark: +(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def main():
    builds = [a.split("=", 1) for a in sys.argv[1:]]
    tabs = [(lab, parse(p)) for lab, p in builds]
    names = sorted(tabs[0][1])
    try:
        dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    except Exception:
        dem = names
    keys = ("VGPRs", "AGPRs", "ScratchSize", "LDS", "Occupancy")
    print("%-10s %5s %5s %7s %6s %4s  kernel" % ("build", "VGPR", "AGPR", "scratch", "LDS", "occ"))
    for n, d in zip(names, dem):
        d = re.sub(r"\(.*", "", d.replace("void ", "").replace("lvx::", ""))
        rows = [(lab, t.get(n)) for lab, t in tabs]
        diff = any(r is not None and r != rows[0][1] for _, r in rows[1:])
        for lab, r in rows:
            if r is None:
                continue
            print("%-10s %5d %5d %7d %6d %4d  %s%s" % ((lab,) + tuple(r.get(k, -1) for k in keys) + (d, "   <-- differs" if diff else "")))
            if not diff:
                break


if __name__ == "__main__":
    main()
