#!/usr/bin/env python3
"""Instruction budget of the row role's loop in cg_herm48_pairs_kernel (csrc/cg_herm.hip), from the gfx950 assembly.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics --cuda-device-only -S -x hip csrc/cg_herm.hip -o cg_herm.s
    python tools/cg48_row_stream.py cg_herm.s '<0, true, false, false, true>' --list
    python tools/cg48_row_stream.py cg_herm.s '<0, true, false, false, true>' --start LBB0_227 --avoid LBB0_225,bb.233,...

(the block labels belong to one compile: --list prints this build's; profiles/r11_cg48_row_stream.txt records the tables of round 10
and round 11 with the labels that were used.)  The tool finds the kernel whose demangled template arguments are given, takes the loop that holds the wave sums (DPP row moves)
and three or six workgroup barriers, and WALKS the path a row wave executes in an iteration of the preconditioned solve: it starts
at --start, falls through, takes every unconditional branch, takes `execnz` and leaves `execz` branches (the row lanes are active),
takes a conditional branch when the block behind it is in --avoid and leaves it when its target is in --avoid or outside the loop,
and stops when it is back at --start.  --avoid names the blocks of the other paths (the "stop" exit, the solve without a
preconditioner, the first application of a warm start): read them off the listing once per build (--list prints the blocks with
their branches).  Instructions are counted by class and by the phase they stand in:

    A           from the start of the row transforms to barrier 1 (the loop's first s_and_saveexec opens it)
    gap         barrier 1 to barrier 2: stop flag, the deferred x update, the copy of p, zeros of the lanes without modes
    D           barrier 2 to the end of the exec-masked block behind it
    updates     to the first DPP move behind D
    sums        the wave sums, to barrier 3
    beta / p    barrier 3 to the next s_and_saveexec (the next A) or the back edge
A body of two iterations is reported per iteration (counts halved).  The phases follow the instructions' positions, so work the
scheduler moved across a marker is counted where it stands.

--barriers 4 is the loop of the arm whose step length comes from a dense wave (round 12): barrier "2b" stands inside D, behind the row
transforms, and D runs on to the end of the exec-masked block behind THAT barrier.

--alpha-slice reports, inside D, the instructions that serve only the sum of <u, A u> and the step length: the backward slice, by
registers, of D's last v_div_fixup_f64 (the quotient), restricted to D; an s_waitcnt or s_nop counts with it when the next
instruction that is neither is in the slice.  (The slice ends at D's first instruction: the numerator and the addresses it reads
are made elsewhere.  Nothing else in D reads a register the slice writes before the slice overwrites it, or the tool says so.)
For the VARIANT 0 kernels: VARIANT 1 divides by sigma^2 in D as well, and the last v_div_fixup_f64 there is not the quotient's.
"""
import argparse
import re
from collections import Counter, OrderedDict

CLASSES = ["fma f64", "mul f64", "add f64", "other f64", "ds_read", "ds_write", "s_barrier", "v_mov_b64", "v_mov_b32", "dpp move",
           "v_cndmask", "v_readlane", "other VALU", "s_waitcnt", "s_nop", "branch", "other SALU"]
PHASES = ["A", "gap", "D", "updates", "sums", "beta / p"]


def classify(ins):
    op = ins.split()[0]
    if "dpp" in op or "row_shr" in ins or "row_bcast" in ins:
        return "dpp move"
    if op.startswith(("v_fma_f64", "v_fmac_f64")):
        return "fma f64"
    if op.startswith("v_mul_f64"):
        return "mul f64"
    if op.startswith("v_add_f64"):
        return "add f64"
    if op.endswith("_f64") or "_f64_" in op:
        return "other f64"
    if op.startswith("ds_read"):
        return "ds_read"
    if op.startswith("ds_write"):
        return "ds_write"
    if op == "s_barrier":
        return "s_barrier"
    if op.startswith("v_mov_b64"):
        return "v_mov_b64"
    if op.startswith("v_mov_b32"):
        return "v_mov_b32"
    if op.startswith("v_cndmask"):
        return "v_cndmask"
    if op.startswith("v_readlane") or op.startswith("v_readfirstlane"):
        return "v_readlane"
    if op.startswith("v_"):
        return "other VALU"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op == "s_nop":
        return "s_nop"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    return "other SALU"


def kernel_body(lines, targs):
    want = re.sub(r"\s", "", targs)
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN4efgp3pcg22cg_herm48_pairs_kernelI(\w+?)EEvNS0_4ArgsE):", l)
        if not m:
            continue
        args = re.findall(r"L[ib](\d)", m.group(2))
        text = "<" + ",".join([args[0]] + ["true" if x == "1" else "false" for x in args[1:]]) + ">"
        if text == want:
            end = next(k for k in range(i, len(lines)) if lines[k].startswith("\t.size\t" + m.group(1)))
            return lines[i:end]
    raise SystemExit("no cg_herm48_pairs_kernel" + targs + " in the file")


def row_loop(body, per_iter=3):
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^\.(LBB\d+_\d+):", l)] if m}
    spans = []
    for i, l in enumerate(body):
        m = re.match(r"^\s+s_c?branch\S*\s+\.(LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), 1 << 30) < i:
            seg = body[labels[m.group(1)]:i + 1]
            nb = sum(1 for x in seg if re.match(r"^\s+s_barrier", x))
            if nb in (per_iter, 2 * per_iter) and any("row_bcast:31" in x for x in seg):
                spans.append((labels[m.group(1)], i))
    if not spans:
        raise SystemExit(f"no loop with wave sums and {per_iter} or {2 * per_iter} barriers")
    return body[min(s[0] for s in spans):max(s[1] for s in spans) + 1]


def blocks_of(loop):
    """ordered name -> instructions; a block starts at a label or at a '; %bb.N:' comment"""
    blocks = OrderedDict()
    cur = None
    for l in loop:
        m = re.match(r"^\.(LBB\d+_\d+):", l) or re.match(r"^; %(bb\.\d+):", l)
        if m:
            cur = m.group(1)
            blocks[cur] = []
        elif cur is not None and re.match(r"^\s+[a-z]", l) and not l.strip().startswith(";"):
            blocks[cur].append(re.sub(r"\s*;.*$", "", l.strip()))
    return blocks


def walk(blocks, start, avoid):
    names = list(blocks)
    path, cur, seen_start = [], start, 0
    for _ in range(10000):
        if cur == start:
            seen_start += 1
            if seen_start == 2:
                return path
        nxt = names[names.index(cur) + 1] if names.index(cur) + 1 < len(names) else None
        jumped = False
        for ins in blocks[cur]:
            path.append(ins)
            m = re.match(r"(s_c?branch\S*)\s+\.(LBB\d+_\d+)", ins)
            if not m:
                continue
            op, tgt = m.groups()
            if tgt not in blocks or tgt in avoid:
                take = False
            elif op == "s_branch" or op.endswith("execnz") or nxt in avoid:
                take = True
            else:
                take = False
            if take:
                cur, jumped = tgt, True
                break
        if not jumped:
            if nxt is None or nxt in avoid:
                raise SystemExit("the walk falls into " + str(nxt) + " behind " + cur)
            cur = nxt
    raise SystemExit("the walk does not come back to " + start)


def phases(path, per_iter=3):
    out, phase = [], "A"
    nbar = 0
    after = {3: {1: "gap", 2: "D", 0: "beta / p"}, 4: {1: "gap", 2: "D", 3: "D", 0: "beta / p"}}[per_iter]
    for ins in path:
        op = ins.split()[0]
        if phase == "beta / p" and op.startswith("s_and_saveexec"):
            phase = "A"
        d_last_block = per_iter == 3 or nbar % per_iter == 3
        if phase == "D" and d_last_block and op == "s_or_b64" and "exec" in ins.split()[1]:
            out.append((phase, ins))
            phase = "updates"
            continue
        if phase == "updates" and ("row_shr" in ins or "row_bcast" in ins):
            phase = "sums"
        out.append((phase, ins))
        if op == "s_barrier":
            nbar += 1
            phase = after[nbar % per_iter]
    return out, nbar


def regs(tok):
    """the 32-bit registers an operand names: v[4:5] -> {v4, v5}, -v[4:5] -> the same, s37, vcc"""
    tok = tok.strip().lstrip("-|").rstrip("|")
    m = re.match(r"^([vs])\[(\d+):(\d+)\]$", tok)
    if m:
        return {f"{m.group(1)}{k}" for k in range(int(m.group(2)), int(m.group(3)) + 1)}
    if re.match(r"^[vs]\d+$", tok):
        return {tok}
    if tok in ("vcc", "exec"):
        return {tok}
    return set()


def defs_uses(ins):
    op, _, rest = ins.partition(" ")
    toks = [t for t in re.split(r"[,\s]+", rest.strip()) if t]
    if op.startswith(("ds_write", "s_waitcnt", "s_nop", "s_barrier", "s_cbranch", "s_branch")):
        return set(), set().union(*[regs(t) for t in toks]) if toks else set()
    ndef = 2 if op.startswith("v_div_scale") else 1
    d = set().union(*[regs(t) for t in toks[:ndef]]) if toks else set()
    u = set().union(*[regs(t) for t in toks[ndef:]]) if len(toks) > ndef else set()
    if "dpp" in op or op.startswith(("v_fmac", "v_div_fmas")):
        u |= d if "dpp" in op or op.startswith("v_fmac") else {"vcc"}
    return d, u


def alpha_slice(d_ins):
    """indices into d_ins (one iteration's D) of the instructions that serve only the quotient"""
    last = max((i for i, x in enumerate(d_ins) if x.startswith("v_div_fixup_f64")), default=None)
    if last is None:
        return set(), []
    want, inslice = set(defs_uses(d_ins[last])[1]), {last}
    for i in range(last - 1, -1, -1):
        d, u = defs_uses(d_ins[i])
        if d & want:
            inslice.add(i)
            want = (want - d) | u
    quiet = ("s_waitcnt", "s_nop")
    for i, x in enumerate(d_ins):
        if x.startswith(quiet):
            nxt = next((k for k in range(i + 1, len(d_ins)) if not d_ins[k].startswith(quiet)), None)
            if nxt in inslice:
                inslice.add(i)
    # a register the slice wrote, read by an instruction outside it before the slice or anyone else rewrites it
    shared, live = [], set()
    for i, x in enumerate(d_ins[:last + 1]):
        d, u = defs_uses(x)
        if i in inslice:
            live |= d
        else:
            if u & live:
                shared.append(x)
            live -= d
    return inslice, shared


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("targs", help="the kernel's template arguments as the demangler prints them, e.g. '<0, true, false>'")
    ap.add_argument("--start", help="label of the block that opens A, e.g. LBB1_225")
    ap.add_argument("--avoid", default="", help="blocks off the steady path, comma separated (LBB1_230, bb.229)")
    ap.add_argument("--list", action="store_true", help="print the loop's blocks with their sizes and branches")
    ap.add_argument("--dump", help="write the walked path to this file")
    ap.add_argument("--barriers", type=int, default=3, choices=(3, 4), help="workgroup barriers per iteration (4: with barrier 2b)")
    ap.add_argument("--alpha-slice", action="store_true", help="inside D, what serves only <u, A u> and the step length")
    a = ap.parse_args()
    loop = row_loop(kernel_body(open(a.asm).read().split("\n"), a.targs), a.barriers)
    blocks = blocks_of(loop)
    if a.list or not a.start:
        for n, b in blocks.items():
            print(f"{n:12s} {len(b):4d}  " + "  ".join(i for i in b if i.startswith(("s_cbranch", "s_branch", "s_barrier"))))
        return
    path = walk(blocks, a.start, set(x for x in a.avoid.split(",") if x))
    tagged, nbar = phases(path, a.barriers)
    per = nbar // a.barriers
    tab = {p: Counter() for p in PHASES}
    for p, ins in tagged:
        tab[p][classify(ins)] += 1
    print(f"static loop: {sum(len(b) for b in blocks.values())} instructions; walked path: {len(path)} instructions, {nbar} barriers"
          f" = {per} iteration(s); per iteration:")
    print(f"{'class':12s}" + "".join(f"{p:>10s}" for p in PHASES) + f"{'total':>10s}")
    for c in CLASSES:
        row = [tab[p][c] / per for p in PHASES]
        if sum(row):
            print(f"{c:12s}" + "".join(f"{v:10g}" for v in row) + f"{sum(row):10g}")
    tot = [sum(tab[p].values()) / per for p in PHASES]
    print(f"{'all':12s}" + "".join(f"{v:10g}" for v in tot) + f"{sum(tot):10g}")
    if a.alpha_slice:
        # D of the first iteration on the path
        first = next(i for i, (p, _) in enumerate(tagged) if p == "D")
        end = next(i for i in range(first, len(tagged)) if tagged[i][0] != "D")
        d_ins = [ins for _, ins in tagged[first:end]]
        inslice, shared = alpha_slice(d_ins)
        cnt = Counter(classify(d_ins[i]) for i in inslice)
        print(f"inside D ({len(d_ins)} instructions): {len(inslice)} serve only <u, A u> and the step length")
        for c in CLASSES:
            if cnt[c]:
                print(f"  {c:12s}{cnt[c]:6d}")
        for x in shared:
            print("  NOT only the quotient's (its result is read outside the slice): " + x)
        for i in sorted(inslice):
            tagged[first + i] = ("D alpha", tagged[first + i][1])
    if a.dump:
        open(a.dump, "w").write("\n".join(f"{p:9s} {i}" for p, i in tagged) + "\n")


if __name__ == "__main__":
    main()
