"""Dev tool: do two versions of the sources compile to the same device code?  Builds the gfx950 listing of frr_api.hip
(_native.HIPCC_FLAGS + --offload-device-only -S) for both and prints, per kernel, how far the instruction text agrees --
equal / equal up to the order of an instruction's operands / the same sequence of mnemonics (registers renamed) / the same
number of instructions per mnemonic / DIFFERS -- with the mnemonic-count deltas and the resource numbers of the kernel's
metadata (VGPRs, SGPRs, scratch, LDS).  Kernels that are equal in everything are only counted.
  python tools/listing_diff.py REV              git revision REV against the working tree
  python tools/listing_diff.py TREE_A TREE_B    two source trees (each a directory, a git revision, or a listing built earlier: *.s)
-v also prints the resource numbers of equal kernels."""
import collections, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from f_renderer_amd import _native

RES = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def tree_of(arg, tmp):
    """a directory as it is; anything else is a git revision, exported"""
    if os.path.isdir(arg) or arg.endswith(".s"):
        return os.path.abspath(arg)
    out = os.path.join(tmp, re.sub(r"\W", "_", arg))
    os.makedirs(out)
    tar = subprocess.run(["git", "-C", ROOT, "archive", arg, "f_renderer_amd/csrc", "include"], check=True, stdout=subprocess.PIPE).stdout
    subprocess.run(["tar", "-x", "-C", out], input=tar, check=True)
    return out


def listing(tree, tmp, tag):
    if tree.endswith(".s"):   # a listing built earlier
        return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(tree).read())
    csrc = os.path.join(tree, "f_renderer_amd", "csrc")
    flags = [f for f in _native.HIPCC_FLAGS if f != "-shared" and not f.startswith(("-L", "-l", "-Wl,", "-DFRR_CSRC_DIR="))]
    out = os.path.join(tmp, tag + ".s")
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc] + flags + ['-DFRR_CSRC_DIR="%s"' % csrc, "--offload-device-only", "-S", "-o", out, os.path.join(csrc, "frr_api.hip")])
    text = open(out).read().replace(tree, "<tree>")
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", text)


def kernels(text):
    """name -> (instruction lines, resource numbers)"""
    lines = text.splitlines()
    res = {}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target:)", text, re.S | re.M):
        d = dict(re.findall(r"^    \.(\w+): +(\S+)$", m.group(0), re.M))
        res[d["name"]] = tuple(int(d[k]) for k in RES)
    out = {}
    for name in res:
        i = next(k for k, l in enumerate(lines) if l.startswith(name + ":"))
        body = []
        for l in lines[i + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            l = l.split(";")[0].strip()
            if l and not l.startswith("."):
                body.append(l)
        out[name] = (body, res[name])
    return out


def agreement(a, b):
    if a == b:
        return "equal"
    ops = lambda l: (l.split()[0], sorted(re.split(r"[,\s]+", l)[1:]))
    if len(a) == len(b) and all(ops(x) == ops(y) for x, y in zip(a, b)):
        return "operand order"
    ma, mb = ([l.split()[0] for l in i] for i in (a, b))
    if ma == mb:
        return "same sequence"
    return "same counts" if sorted(ma) == sorted(mb) else "DIFFERS"


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    verbose = "-v" in sys.argv[1:]
    if len(args) == 1:
        args.append(ROOT)
    if len(args) != 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        ta, tb = (listing(tree_of(a, tmp), tmp, t) for a, t in zip(args, "ab"))
    print("listing lines: %d vs %d" % (ta.count("\n"), tb.count("\n")))
    ka, kb = kernels(ta), kernels(tb)
    for n in sorted(set(ka) ^ set(kb)):
        print("only in %s: %s" % ("A" if n in ka else "B", n))
    tally = collections.Counter()
    for n in ka:
        if n not in kb:
            continue
        (ia, ra), (ib, rb) = ka[n], kb[n]
        state = agreement(ia, ib)
        tally[state] += 1
        if ra != rb:
            tally["resources differ"] += 1
        if state == "equal" and ra == rb and not verbose:
            continue
        print("%-13s %s" % (state, n))
        print("    " + "  ".join("%s %d%s" % (k, x, "" if x == y else " -> %d" % y) for k, x, y in zip(RES, ra, rb)))
        ca, cb = (collections.Counter(l.split()[0] for l in i) for i in (ia, ib))
        d = {m: cb[m] - ca[m] for m in set(ca) | set(cb) if ca[m] != cb[m]}
        print("    instructions %d -> %d  mnemonic deltas: %s" % (len(ia), len(ib), " ".join("%s %+d" % kv for kv in sorted(d.items())) or "none"))
    print("%d kernels: " % len(ka) + ", ".join("%d %s" % (v, k) for k, v in tally.items()))


if __name__ == "__main__":
    main()
