"""Static instruction counts of kernels in an assembly listing (`hipcc ... --cuda-device-only -S`), and whether a kernel's listing equals
the same kernel's in a second listing:
    python tools/listing_counts.py now.s [parent.s] SUBSTRING [SUBSTRING ...]
A kernel is chosen by a substring of its mangled name.  Lines are counted, not what a wave executes; every s_* line counts as SALU (waits
included); lane moves = v_readlane / v_writelane / v_readfirstlane.  The comparison strips comments and blank lines."""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            code = ln.split(";")[0].strip()
            if code.startswith(".Lfunc_end"):
                out[name], name = body, None
            elif code and not code.startswith("."):
                body.append(code)
    return out


def counts(body):
    op = [b.split()[0] for b in body if not b.endswith(":")]
    n = lambda f: sum(1 for o in op if f(o))
    return dict(instr=len(op), VALU=n(lambda o: o.startswith("v_")), SALU=n(lambda o: o.startswith("s_")),
                cbranch=n(lambda o: o.startswith("s_cbranch")), barrier=n(lambda o: o == "s_barrier"),
                v_div=n(lambda o: o.startswith("v_div_")),
                lane=n(lambda o: o.startswith(("v_readlane", "v_writelane", "v_readfirstlane"))),
                DPP=n(lambda o: o.endswith("_dpp")),
                vmem=n(lambda o: o.startswith(("buffer_", "global_")) and "atomic" not in o),
                atomics=n(lambda o: "atomic" in o), s_sleep=n(lambda o: o == "s_sleep"))


files = [a for a in sys.argv[1:] if a.endswith(".s")]
subs = [a for a in sys.argv[1:] if not a.endswith(".s")]
ks = [kernels(f) for f in files]
for s in subs:
    for f, k in zip(files, ks):
        hit = [n for n in k if s in n]
        if len(hit) != 1:
            sys.exit(f"{f}: {len(hit)} kernels match {s!r}")
        c = counts(k[hit[0]])
        print(f"{f:24s} {s:40s} " + " ".join(f"{a} {b}" for a, b in c.items()))
    if len(ks) == 2:
        a, b = ([x for n, x in k.items() if s in n][0] for k in ks)
        print(f"{'':24s} {s:40s} listings identical: {a == b}")
