"""CPU: compare two device assembly files of one translation unit kernel by kernel (the gate of a refactor that must not change the code).
python tools/asm_diff.py parent.s branch.s [name filter]
The files come from `hipcc <the Makefile's flags> --cuda-device-only -S file.hip -o file.s`.  Per kernel symbol, one of
  identical            the instruction text is equal (comments, blank lines, the numbering of local labels and the __hip_cuid name aside)
  outside loops only   the .amdhsa_ descriptor, the metadata entry and the multiset of mnemonics are equal, and the loops (every basic block that
                       lies on a cycle of the control-flow graph) hold the same instructions in the same order once register numbers are normalised
  differs inside a loop    some loop's normalised instruction sequence is not equal
  differs              the loops are equal, but the descriptor / metadata or the mnemonic multiset is not (the columns after the verdict say which)
Exit status 1 if any kernel gets one of the last two or exists in one file only."""
import collections
import re
import subprocess
import sys

REG = re.compile(r"\b([vsa])(\d+|\[\d+:\d+\])")
LABEL = re.compile(r"\.L[A-Za-z_]*\d+(_\d+)?")
BRANCH = re.compile(r"^s_c?branch\w*\s+(\S+)$")


def width(m):
    r = m.group(2)
    if r[0] != "[":
        return m.group(1)
    lo, hi = r[1:-1].split(":")
    return f"{m.group(1)}[{int(hi) - int(lo) + 1}]"


def parse(path):
    """-> {symbol: (body lines, descriptor lines, metadata lines)}"""
    lines = [re.sub(r"\s*(;|//).*", "", l).strip() for l in open(path)]
    lines = [re.sub(r"__hip_cuid_\w+", "__hip_cuid", l) for l in lines if l]
    desc, meta, body = {}, {}, {}
    i = 0
    while i < len(lines):
        l = lines[i]
        if l.startswith(".amdhsa_kernel "):
            j = lines.index(".end_amdhsa_kernel", i)
            desc[l.split()[1]] = lines[i + 1:j]
            i = j
        elif l.startswith("- .agpr_count:") or l.startswith("- .args:"):           # one kernel's entry of amdhsa.kernels
            j = i + 1
            while j < len(lines) and not lines[j].startswith("- .a") and not lines[j].startswith("amdhsa."):
                j += 1
            ent = lines[i:j]
            name = [x.split(":", 1)[1].strip() for x in ent if x.startswith(".name:")]
            if name:
                meta[name[0]] = ent
            i = j - 1
        i += 1
    for sym in desc:
        s = lines.index(sym + ":")
        e = next(k for k in range(s, len(lines)) if lines[k].startswith(".Lfunc_end"))
        body[sym] = [x for x in lines[s + 1:e] if not (x.startswith(".") and not x.endswith(":"))]   # instructions and labels, no directives
    return {sym: (body[sym], desc[sym], meta.get(sym, [])) for sym in desc}


def relabel(body):
    """local labels renumbered in order of first appearance"""
    names = {}
    return [LABEL.sub(lambda m: names.setdefault(m.group(0), f".L{len(names)}"), l) for l in body]


def loops(body):
    """the instructions that lie on a cycle of the control-flow graph, in layout order, registers normalised.  (A label and the last branch back to
    it delimit the same code as long as the loop is laid out in one piece; hipcc also puts rarely taken blocks of a loop behind the kernel's
    epilogue, and the layout span then takes the epilogue in: the cycle is what a loop executes.)"""
    cuts = {0}
    for k, l in enumerate(body):
        if l.endswith(":"):
            cuts.add(k)
        elif BRANCH.match(l) or l.startswith(("s_endpgm", "s_setpc")):
            cuts.add(k + 1)
    starts = sorted(c for c in cuts if c < len(body))
    ends = starts[1:] + [len(body)]
    at = {}
    for i, s in enumerate(starts):
        while s < len(body) and body[s].endswith(":"):
            at[body[s][:-1]] = i
            s += 1
    succ = []
    for i, e in enumerate(ends):
        last, m = body[e - 1], BRANCH.match(body[e - 1])
        fall = [i + 1] if i + 1 < len(starts) else []
        if m:
            succ.append([at[m.group(1)]] + (fall if last.startswith("s_cbranch") else []))
        else:
            succ.append([] if last.startswith(("s_endpgm", "s_setpc")) else fall)
    # a block is on a cycle iff it reaches itself
    on_cycle = []
    for i in range(len(starts)):
        seen, todo = set(), list(succ[i])
        while todo and i not in seen:
            v = todo.pop()
            if v not in seen:
                seen.add(v)
                todo.extend(succ[v])
        if i in seen:
            on_cycle.append(i)
    return relabel([REG.sub(width, x) for i in on_cycle for x in body[starts[i]:ends[i]]]), len(on_cycle)


def mnemonics(body):
    return collections.Counter(l.split()[0] for l in body if not l.endswith(":"))


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    flt = sys.argv[3] if len(sys.argv) > 3 else ""
    syms = sorted(set(a) | set(b))
    dem = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.splitlines()
    rows, bad = [], 0                                     # (a c++filt that does not know _Float16 / __bf16 leaves those symbols mangled)
    for sym, name in zip(syms, dem):
        name = re.sub(r"^void ", "", name).split("(")[0]
        if flt and flt not in name:
            continue
        if sym not in a or sym not in b:
            rows.append(f"{name[:100]:100s} only in {'the first' if sym in a else 'the second'} file")
            bad += 1
            continue
        (ba, da, ma), (bb, db, mb) = a[sym], b[sym]
        same_desc, same_mn = da == db and ma == mb, mnemonics(ba) == mnemonics(bb)
        (la, na), (lb, _) = loops(ba), loops(bb)
        if same_desc and relabel(ba) == relabel(bb):
            verdict = "identical"
        elif same_desc and same_mn and la == lb:
            verdict = "outside loops only"
        else:
            verdict = "differs inside a loop" if la != lb else "differs"
            bad += 1
        rows.append(f"{name[:100]:100s} {verdict:22s} descriptor {'same' if same_desc else 'DIFFERS'}  mnemonics {'same' if same_mn else 'DIFFER'}  "
                    f"blocks in loops {na}  instructions {sum(mnemonics(ba).values())}")
    print("\n".join(sorted(rows)))
    print(f"{len(rows)} kernels, {sum('identical' in r for r in rows)} identical, {sum('outside loops only' in r for r in rows)} outside loops only, {bad} failing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
