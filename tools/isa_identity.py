#!/usr/bin/env python3
"""Is the device code of two source trees the same, kernel by kernel?

    python tools/isa_identity.py PARENT_TREE NEW_TREE [--jobs N] [--out FILE]

For every .hip in SRCS of each tree's orb_slam3_fast_amd/csrc/Makefile, the device side is compiled to assembly with the
Makefile's FLAGS (hipcc -S --cuda-device-only), the text is cut at function symbols, comments are stripped and local labels
are renumbered in order of appearance.  Kernels (and the device functions that were not inlined) are matched by SYMBOL, not
by file, so code may move between translation units.  Per symbol two things are compared: the instruction text and, for
kernels, the .amdhsa_* block (registers, LDS, scratch, kernarg size).  A file whose source is byte-identical in both trees
must also give the same assembly as a whole (the __hip_cuid_* symbol aside).  The tool only diffs; it looks for no
particular instruction.  One line per symbol, a summary, exit status 1 on any difference.  Needs no GPU.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("orb_slam3_fast_amd", "csrc")


def make_vars(tree):
    """SRCS and FLAGS of the tree's Makefile (continuation lines joined, $(ARCH) / $(HIPCC) expanded)."""
    text = open(os.path.join(tree, CSRC, "Makefile")).read().replace("\\\n", " ")
    var = {}
    for m in re.finditer(r"^([A-Z_]+)\s*\??=\s*(.*)$", text, re.M):
        var.setdefault(m.group(1), m.group(2).strip())
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), s)
    return var.get("HIPCC", "hipcc"), expand(var["FLAGS"]).split(), var["SRCS"].split()


def compile_tree(tree, outdir, jobs):
    hipcc, flags, srcs = make_vars(tree)
    hipcc = os.environ.get("HIPCC", hipcc)

    def one(src):
        out = os.path.join(outdir, src[:-4] + ".s")
        cmd = [hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, src]
        r = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("%s failed:\n%s" % (" ".join(cmd), r.stdout))
        return src, out

    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as ex:
        return dict(ex.map(one, srcs))


LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def clean(lines):
    """comments and blank lines out, local labels renumbered in order of first appearance"""
    names = {}
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip():
            continue
        out.append(LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), ln))
    return out


def parse(path):
    """{symbol: (instruction text, amdhsa block or None)} and the whole file's cleaned text"""
    lines = open(path).read().split("\n")
    funcs = [m.group(1) for ln in lines for m in [re.match(r"\s*\.type\s+(\S+),@function", ln)] if m]
    start = {}
    for i, ln in enumerate(lines):
        m = re.match(r"([A-Za-z_$][\w$.]*):", ln)
        if m and m.group(1) in funcs:
            start[m.group(1)] = i
    syms = {}
    for f in funcs:
        i = start[f]
        end = next(j for j in range(i, len(lines)) if re.match(r"\s*\.size\s+%s," % re.escape(f), lines[j]))
        body = lines[i:end]
        hsa = None
        for j, ln in enumerate(body):
            if re.match(r"\s*\.amdhsa_kernel\s", ln):
                k = next(q for q in range(j, len(body)) if ".end_amdhsa_kernel" in body[q])
                hsa = [x.strip() for x in body[j:k + 1]]
                body = body[:j] + body[k + 1:]
                break
        syms[f] = (clean(body), hsa)
    whole = clean(ln for ln in lines if "__hip_cuid_" not in ln)
    return syms, whole


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    report = []
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        asm = {}
        for tag, tree in (("parent", a.parent), ("new", a.new)):
            d = os.path.join(tmp, tag)
            os.mkdir(d)
            asm[tag] = compile_tree(tree, d, a.jobs)
        parsed = {tag: {src: parse(p) for src, p in asm[tag].items()} for tag in asm}
    where = {tag: {s: src for src, (syms, _) in parsed[tag].items() for s in syms} for tag in parsed}
    code = {tag: {s: v for (syms, _) in parsed[tag].values() for s, v in syms.items()} for tag in parsed}
    for s in sorted(set(code["parent"]) | set(code["new"])):
        if s not in code["new"] or s not in code["parent"]:
            report.append("MISSING in %s   %s  (%s)" % ("new" if s in code["parent"] else "parent", s, where["parent"].get(s) or where["new"].get(s)))
            bad += 1
            continue
        (tp, hp), (tn, hn) = code["parent"][s], code["new"][s]
        kind = "kernel  " if hp is not None else "function"
        verdict = "identical" if tp == tn and hp == hn else "DIFFERS (%s)" % ", ".join(
            w for w, d in (("text", tp != tn), ("resources", hp != hn)) if d)
        bad += verdict != "identical"
        moved = where["parent"][s] if where["parent"][s] == where["new"][s] else "%s -> %s" % (where["parent"][s], where["new"][s])
        report.append("%-9s %s %s  (%s)" % (verdict, kind, s, moved))
    for src in sorted(set(parsed["parent"]) & set(parsed["new"])):
        same_src = open(os.path.join(a.parent, CSRC, src), "rb").read() == open(os.path.join(a.new, CSRC, src), "rb").read()
        same_asm = parsed["parent"][src][1] == parsed["new"][src][1]
        if same_src:
            report.append("file %-28s source untouched, assembly as a whole %s" % (src, "identical" if same_asm else "DIFFERS"))
            bad += not same_asm
        else:
            report.append("file %-28s source changed, assembly as a whole %s" % (src, "identical" if same_asm else "differs (see its symbols above)"))
    for tag, other in (("parent", "new"), ("new", "parent")):
        for src in sorted(set(parsed[tag]) - set(parsed[other])):
            report.append("file %-28s only in the %s tree" % (src, tag))
    nk = sum(1 for s in code["new"] if code["new"][s][1] is not None)
    report.append("%d symbols (%d kernels) in the new tree, %d in the parent; %d difference%s"
                  % (len(code["new"]), nk, len(code["parent"]), bad, "" if bad == 1 else "s"))
    text = "\n".join(report) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
