#!/usr/bin/env python3
"""Static instruction census of the matcher's stage kernel, k_match_split<8, 4, 3>, made without a GPU.

Compiles k_verify.hip to gfx950 assembly with the product flags (csrc/Makefile: COMMON + CANON, as tools/pk_isa_scan.py
does), cuts the kernel into the regions a wavefront walks through and prints, per region, its vector (VALU, MFMA), scalar,
LDS and memory instructions, then the modelled vector instructions of ONE wavefront for frames of K = 500, 512 and 1 000
features on both sides.  The kernel is bound by vector instruction issue, so this count is its cost.

The regions are found from the instruction stream, not from label numbers:
  * basic blocks are cut at labels and behind branches; a block that branches to itself and holds MFMAs is a scan loop,
    the one with 16 MFMAs is the scan of a 4-tile column group (the only groups a wavefront runs at these K);
  * a group's region is what the topmost block dominates that dominates this loop alone and is itself neither a scan nor
    a decode (v_ceil_f32) nor a claim (ds_add); inside it: in front of the loop (the "to" tiles loaded and spread, the
    origin tuple), the loop, what lies on a cycle through the loop (the ragged tile as a second pass), what follows it
    (blocks with MFMAs there = an unpipelined ragged tile; the rest = drain, decode, NNDR, claims);
  * the repair of the second best (mf_repair_accept, mf_repair_d2) is a region of its own behind the scan loop: a block
    there that branches to itself and holds v_bcnt_u32_b32 is a repair loop (4 of a class's rows per trip, 4 trips), and
    its region is what the topmost block dominates that dominates it and is neither a decode (v_ceil_f32) nor a claim
    (ds_add).  A group has ONE copy: the hand-over of pass 1's columns to free lanes, the loop of the half-row certificate
    (the repair loop with the fewest v_bcnt_u32_b32) and the exact path for uncertified lanes (the other loop and what
    the topmost block dominates that dominates it and not the certificate's loop);
  * the two barriers in front of and behind the scans cut the rest: prologue + staging, scan set-up, the loop over a
    wavefront's groups, the hand-over of the rejected count, the list compaction and the header.
Loop bodies other than the scan loop are counted once.  The model adds up what every wavefront of a pair issues; what only
lane 0 of the workgroup runs behind the compaction (header, pass state, the result of a pair that has no estimate) and
the paths taken by few pairs are listed and left out of it.  model_valu is a wavefront none of whose decode passes
repairs (no lane accepts against the optimistic second best: every pass of a pair of unrelated frames);
model_valu_repaired one whose every group repairs ONCE, both passes' columns merged into one set of lanes and all of them
certified (the repair region less its exact path, the certificate's loop four times).  Assembly from before the certificate
(one kind of repair loop, one copy per decode pass) is modelled as it was: every pass repairing, its loop four times.
The EXECUTED model (docs/match_tail.md) adds what that leaves out: the trips of the loops outside the scan as a function of
Kf (a prologue loop that loads runs once per 128 "from" rows and global load in it, one that only zeroes once per 256; the
compaction once per 256, as a loop or as unrolled trips cut at their markers), lane 0's tail split by what its blocks hold,
and, for a launch of given survivors, non-survivors and void slots, the total of vector and matrix instructions -- the
counter SQ_INSTS_VALU holds both.
  tools/match_isa_census.py [--asm FILE | --figures FILE] [--json] [--mix Kf,Kt,survivors,non_survivors,void ...]
--asm: read an assembly file made before (the parent commit's, say) instead of compiling.
--figures: run the executed model on the figures of an earlier --json output.  --mix: default the benchmark's launch."""
import argparse, collections, json, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi_robot_slam_separators_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", "-Wno-pass-failed",
         "-fno-slp-vectorize", "-ffp-contract=off", "-fno-vectorize"]
SPLIT = "13k_match_splitILi8ELi4ELi3EE"
FUSED = "14k_verify_fusedILi8ELi0ELb0EE"
KINDS = ("valu", "mfma", "salu", "lds", "vmem")
BENCH_MIX = "500,500,2000,8000,1506"     # python bench.py: 10 000 pairs, one in five true, on a grid of 11 506 slots


def compile_asm(path):
    subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-S", "--cuda-device-only", os.path.join(CSRC, "k_verify.hip"), "-o", path],
                   check=True, stderr=subprocess.DEVNULL)


def kind(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_"):
        return "salu"
    return None


def function_lines(lines, tag):
    """The instruction and label lines of the kernel whose mangled name holds `tag`."""
    out, on = [], False
    for ln in lines:
        if re.match(r"^_Z\w+:", ln):
            on = tag in ln
            continue
        if on:
            if ln.startswith(".Lfunc_end"):
                break
            out.append(ln.rstrip("\n"))
    if not out:
        sys.exit("kernel %s not found in the assembly" % tag)
    return out


def resources(lines, tag):
    """Registers, scratch and occupancy the compiler reports for the kernel."""
    r, seen = {}, False
    for ln in lines:                 # the "; Kernel info:" comments behind the kernel's descriptor hold the final figures
        if ln.startswith("\t.amdhsa_kernel"):
            seen = tag in ln
        m = re.match(r"; (NumVgprs|ScratchSize|Occupancy): (\d+)", ln)
        if m and seen:
            r[m.group(1)] = int(m.group(2))
            seen = m.group(1) != "Occupancy"
    if len(r) != 3:
        sys.exit("kernel info of %s not found in the assembly" % tag)
    return {"vgprs": r["NumVgprs"], "scratch_bytes": r["ScratchSize"], "occupancy": r["Occupancy"]}


class Block:
    def __init__(self, name):
        self.name, self.ins, self.succ, self.falls = name, [], [], True

    def count(self, ins=None):
        c = collections.Counter()
        for op in (self.ins if ins is None else ins):
            k = kind(op)
            if k:
                c[k] += 1
        return c

    def has(self, prefix):
        return any(op.startswith(prefix) for op in self.ins)


def blocks_of(fn):
    blocks, cur, n = [], Block("entry"), 0
    blocks.append(cur)
    for ln in fn:
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            cur = Block(m.group(1))
            blocks.append(cur)
            continue
        t = ln.strip()
        if not ln.startswith("\t") or t.startswith((".", ";")):
            continue
        toks = t.split()
        op = toks[0]
        cur.ins.append(op)
        if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
            if op.startswith(("s_cbranch", "s_branch")):
                cur.succ.append(toks[1])
            cur.falls = op.startswith("s_cbranch")
            n += 1
            cur = Block("%s+%d" % (blocks[-1].name.split("+")[0], n))       # the fall-through behind a branch
            cur_prev = blocks[-1]
            blocks.append(cur)
            if cur_prev.falls:
                cur_prev.succ.append(cur.name)
    for i, b in enumerate(blocks):                                          # a block that runs into the next label
        if b.falls and i + 1 < len(blocks) and blocks[i + 1].name not in b.succ and not (b.ins and b.ins[-1].startswith("s_cbranch")):
            if not b.ins or not b.ins[-1].startswith(("s_branch", "s_endpgm", "s_setpc")):
                b.succ.append(blocks[i + 1].name)
    return blocks


def reach(start, succ, allowed=None, skip=()):
    seen, todo = set(), list(start)
    while todo:
        x = todo.pop()
        for y in succ.get(x, ()):
            if y in seen or y in skip or (allowed is not None and y not in allowed):
                continue
            seen.add(y)
            todo.append(y)
    return seen


def dominators(names, succ, entry):
    pred = collections.defaultdict(set)
    for a in names:
        for b in succ[a]:
            pred[b].add(a)
    live = reach([entry], succ) | {entry}
    dom = {n: set(live) for n in live}
    dom[entry] = {entry}
    changed = True
    while changed:
        changed = False
        for n in names:
            if n not in live or n == entry:
                continue
            ps = [dom[p] for p in pred[n] if p in live]
            new = set.intersection(*ps) | {n} if ps else {n}
            if new != dom[n]:
                dom[n], changed = new, True
    return dom, live


def census(fn):
    blocks = blocks_of(fn)
    by = {b.name: b for b in blocks}
    names = [b.name for b in blocks]
    succ = {b.name: [s for s in b.succ if s in by] for b in blocks}
    back = collections.defaultdict(set)
    for a in names:
        for b in succ[a]:
            back[b].add(a)
    dom, live = dominators(names, succ, "entry")
    scans = [n for n in names if n in live and n in succ[n] and by[n].has("v_mfma")]
    scan4 = [n for n in scans if by[n].count()["mfma"] == 16]
    if len(scan4) != 1:
        sys.exit("expected one scan loop with 16 MFMAs, found %d" % len(scan4))
    scan4 = scan4[0]
    dominated = lambda d: set(n for n in live if d in dom[n])

    def region_of(loop):
        head, cand = loop, loop
        while True:
            ups = [d for d in dom[cand] if d != cand and dom[d] == dom[cand] - {cand}]      # the immediate dominator
            if not ups:
                break
            cand = ups[0]
            b = by[cand]
            if b.has("v_mfma") or b.has("v_ceil_f32") or b.has("ds_add") or any(s != loop and s in dominated(cand) for s in scans):
                break
            head = cand
        return head, dominated(head)

    regions = {s: region_of(s) for s in scans}
    head4, reg4 = regions[scan4]
    in_groups = set().union(*[r for _, r in regions.values()])
    inner = {n: [s for s in succ[n] if s in reg4 and s != head4] for n in reg4}
    inner_back = collections.defaultdict(list)
    for a, ss in inner.items():
        for b in ss:
            inner_back[b].append(a)
    after_loop = reach([scan4], inner) - {scan4}
    before_loop = reach([scan4], inner_back) - {scan4}
    cyc = after_loop & before_loop
    pre = (before_loop | {head4}) - cyc - {scan4}
    post = after_loop - cyc
    ragged = set(n for n in post if by[n].has("v_mfma"))
    repair_loops = [n for n in post if n in succ[n] and by[n].has("v_bcnt_u32_b32")]
    repair = set()
    for lp in repair_loops:
        head = lp
        while True:
            ups = [d for d in dom[head] if d != head and dom[d] == dom[head] - {head}]
            if not ups or ups[0] not in post or by[ups[0]].has("v_ceil_f32") or by[ups[0]].has("ds_add") or by[ups[0]].has("v_mfma"):
                break
            head = ups[0]
        repair |= dominated(head) & post
    # the rest of the kernel, cut at its first two barriers that lie outside the groups
    bars = [n for n in names if n in live and by[n].has("s_barrier") and n not in in_groups]
    if len(bars) < 2:
        sys.exit("expected a barrier in front of and one behind the scans")
    bar1, bar2 = bars[0], bars[1]
    reaches_scan = reach(scans, back) | set(scans)
    from_scan = reach(scans, succ)
    dispatch = (reaches_scan & from_scan) - in_groups
    front = set(n for n in live if n in reaches_scan and n not in from_scan and n not in in_groups)
    to_bar1 = (reach([bar1], back) | {bar1}) & front
    setup = front - to_bar1
    behind = set(n for n in live if n in from_scan and n not in reaches_scan and n not in in_groups)
    to_bar2 = (reach([bar2], back) | {bar2}) & behind
    # behind the second barrier: the compaction loop runs up to the last barrier; what follows is lane 0's (header, pass
    # state, the result of a pair without an estimate) or runs for few pairs (the count of finite points), and so do the
    # blocks no scan leads to (a pair whose slots do not exist)
    to_last = (reach([bars[-1]], back) | {bars[-1]}) & (behind - to_bar2)
    rest = set(n for n in live if n not in reaches_scan and n not in from_scan) | (behind - to_bar2 - to_last)

    def cut(name, first):            # a barrier block's instructions in front of / behind its first barrier
        ins = by[name].ins
        i = next(k for k, op in enumerate(ins) if op.startswith("s_barrier"))
        return ins[:i + 1] if first else ins[i + 1:]

    def total(bs, extra=()):
        c = collections.Counter()
        for n in bs:
            c += by[n].count()
        for ins in extra:
            c += Block("").count(ins)
        return c

    rows = collections.OrderedDict()
    rows["prologue + staging of the \"from\" block (loop bodies once)"] = total(to_bar1 - {bar1}, [cut(bar1, True)])
    rows["scan set-up in front of the groups"] = total(setup, [cut(bar1, False)])
    rows["loop over a wavefront's groups (per group)"] = total(dispatch)
    rows["4-tile group: \"to\" tiles loaded and spread, origin tuple"] = total(pre)
    rows["full-tile loop body (per 32 \"from\" rows)"] = total([scan4])
    tail = total(ragged) + total(cyc) + (total([scan4]) if cyc and not ragged else collections.Counter())
    rows["ragged last tile%s" % (" (second pass over the loop body)" if cyc and not ragged else "")] = tail
    rows["drain, decode, NNDR, claims"] = total(post - ragged - repair)
    rows["second best decided again (hand-over, certificate, exact path; loop bodies once)"] = total(repair)
    rows["rejected count handed over"] = total(to_bar2 - {bar2}, [cut(bar2, True)])
    rows["list compaction (loop body once)"] = total(to_last - {bar2}, [cut(bar2, False)] if bar2 != bars[-1] else [])
    rows["behind it: lane 0's header and result, rare paths (not in the model)"] = total(rest, [cut(bar2, False)] if bar2 == bars[-1] else [])
    keys = list(rows)
    once = sum(rows[k]["valu"] for k in (keys[0], keys[1], keys[8], keys[9]))
    bcnts = {lp: sum(op.startswith("v_bcnt_u32_b32") for op in by[lp].ins) for lp in repair_loops}
    shapes = {lp: (bcnts[lp], by[lp].count()["lds"], by[lp].count()["valu"]) for lp in repair_loops}
    if len(set(shapes.values())) > 1 and len(set(bcnts.values())) == 1:
        # two kinds of repair loop are there, and the rule that tells them apart does not: no silent fall-back to the old model
        sys.exit("repair loops of different shape with the same number of v_bcnt_u32_b32: cannot tell the certificate's loop")
    cert = [lp for lp in repair_loops if bcnts[lp] == min(bcnts.values()) and len(set(bcnts.values())) > 1]
    if cert:                       # one merged, certified repair: not the exact path, 4 trips through the certificate's loop
        exact_path = set()
        for lp in repair_loops:
            if lp in cert:
                continue
            head = lp
            while True:
                ups = [d for d in dom[head] if d != head and dom[d] == dom[head] - {head}]
                if not ups or ups[0] not in repair or any(c in dominated(ups[0]) for c in cert):
                    break
                head = ups[0]
            exact_path |= dominated(head) & repair
        rows = collections.OrderedDict(
            (k2, v2) for k, v in rows.items()
            for k2, v2 in ([(k, v), ("... of which the exact path of uncertified lanes", total(exact_path))] if k == keys[7] else [(k, v)]))
        rep = total(repair - exact_path)["valu"] + 3 * total(cert)["valu"]
    else:                          # before the certificate: every pass repairing, 4 trips through its loop
        rep = rows[keys[7]]["valu"] + 3 * total(repair_loops)["valu"]
    per_group = rows[keys[2]]["valu"] + rows[keys[3]]["valu"] + rows[keys[6]]["valu"]
    loop, rag = rows[keys[4]]["valu"], rows[keys[5]]["valu"]

    def model(k, repaired=False):
        tiles = (((k + 31) // 32) + 3) // 4            # column tiles of wavefront 0 (4 wavefronts per pair)
        if tiles % 4:
            sys.exit("K = %d: not only 4-tile groups" % k)
        return once + (tiles // 4) * (per_group + (rep if repaired else 0) + (k // 32) * loop + (rag if k % 32 else 0))

    # ---- the EXECUTED count: trip counts of the loops outside the scan, lane 0's tail by path (docs/match_tail.md) ------
    def loops_of(region):            # the sets of blocks of `region` that lie on a cycle inside it, one set per loop
        region, out, seen = set(region), [], set()
        sub = {n: [s for s in succ[n] if s in region] for n in region}
        for n in names:
            if n in region and n not in seen:
                fwd = reach([n], sub)
                if n in fwd:
                    scc = set(m for m in fwd if n in reach([m], sub))
                    seen |= scc
                    out.append(scc)
        return out

    n_ops = lambda bs, prefix: sum(op.startswith(prefix) for n in bs for op in by[n].ins)
    # prologue: a loop that loads stages 256 sixteen-byte items per global load and trip (2 Kf items of 256-bit rows), one
    # that does not zeroes 256 counters per trip; the report of a pair whose slots do not exist (the blocks that store to
    # global memory in front of the first barrier) belongs to the void path
    pro = to_bar1 - {bar1}
    void_report = set(n for n in pro if by[n].has("global_store"))
    pro_loops = loops_of(pro - void_report)
    in_pro_loops = set().union(*pro_loops) if pro_loops else set()
    ex_pro = {"base": total(pro - void_report - in_pro_loops, [cut(bar1, True)])["valu"],
              "loops": [{"valu": total(lp)["valu"], "rows_per_trip": 128 * n_ops(lp, "global_load") or 256} for lp in pro_loops]}
    # compaction: from the second barrier to the last barrier in front of the count of finite points (v_cmp_class_f32)
    tail_all = behind - to_bar2
    fin_blocks = set(n for n in tail_all if by[n].has("v_cmp_class_f32"))
    fin = set(fin_blocks)
    for lp in loops_of(tail_all):
        if lp & fin_blocks:
            fin |= lp
    to_fin = reach(fin, back) if fin else set()
    cbars = [n for n in bars if n in tail_all and n not in fin and (n in to_fin or not fin)]
    if not cbars:
        sys.exit("no barrier of the list compaction found")
    comp = ((reach([cbars[-1]], back) | {cbars[-1]}) & tail_all) - fin
    comp_loops = loops_of(comp)
    ex_comp = {"always": 0, "trips": [], "loop": 0}
    first_bar_extra = [cut(bar2, False)] if bar2 not in comp else []
    if comp_loops:                   # a loop of one trip per 256 "from" rows
        in_l = set().union(*comp_loops)
        ex_comp["always"] = total(comp - in_l, first_bar_extra)["valu"]
        ex_comp["loop"] = total(in_l)["valu"]
    else:                            # unrolled: all ballots (one s_bcnt1_i32_b64 per trip), ONE barrier, all writes (one
        order = [n for n in names if n in comp]          # v_mbcnt_hi_u32_b32 per trip); a trip's blocks end at its marker
        cut_at = order.index(cbars[0])
        trips = []
        always = total([], first_bar_extra)["valu"]
        for phase, marker in ((order[:cut_at + 1], "s_bcnt1_i32_b64"), (order[cut_at + 1:], "v_mbcnt_hi_u32_b32")):
            n_mark = sum(by[n].has(marker) for n in phase)
            k = 0
            per = [0] * n_mark
            for n in phase:
                if k < n_mark:
                    per[k] += by[n].count()["valu"]
                else:
                    always += by[n].count()["valu"]
                k += by[n].has(marker)
            trips.append(per)
        if len(trips[0]) != len(trips[1]) or not trips[0]:
            sys.exit("unrolled compaction: %d ballots, %d writes" % (len(trips[0]), len(trips[1])))
        ex_comp["always"], ex_comp["trips"] = always, [a + b for a, b in zip(*trips)]
    # lane 0's tail: what is left behind the compaction, by what it holds
    tail = tail_all - comp - fin
    pose = set(n for n in tail if any("_f64" in op for op in by[n].ins))       # the pose of an estimate: no null pass runs it
    alone = set(n for n in live if n not in reaches_scan and n not in from_scan) | void_report
    ex_tail = {"lane0": total(tail - pose)["valu"], "finite_count": total(fin)["valu"], "pose": total(pose)["valu"],
               "void_only": total(alone)["valu"], "entry": by["entry"].count()["valu"]}
    ex = {"prologue": ex_pro, "setup": rows[keys[1]]["valu"], "per_group": per_group, "loop": loop, "ragged": rag, "repair": rep,
          "handover": rows[keys[8]]["valu"], "compaction": ex_comp, "tail": ex_tail}

    ks = (500, 512, 1000)
    return rows, {k: model(k) for k in ks}, {k: model(k, True) for k in ks}, total(live), ex


def executed(ex, kf, kt):
    """Vector instructions one wavefront of a pair EXECUTES, from the figures census() took from the assembly: the regions
    outside the scan with their trip counts, the groups of wavefront 0, and lane 0's tail by path (first wavefront only)."""
    ceil = lambda a, b: (a + b - 1) // b
    pro = ex["prologue"]["base"] + sum(l["valu"] * ceil(kf, l["rows_per_trip"]) for l in ex["prologue"]["loops"])
    ntrip = ceil(kf, 256)
    c = ex["compaction"]
    if c["trips"] and ntrip > len(c["trips"]):
        sys.exit("Kf = %d: more compaction trips than the kernel has" % kf)
    comp = c["always"] + sum(c["trips"][:ntrip]) + c["loop"] * ntrip
    tiles = ceil(ceil(kt, 32), 4) if kf > 0 else 0
    if tiles % 4:
        sys.exit("Kt = %d: not only 4-tile groups" % kt)
    groups = tiles // 4
    scan = groups * (ex["per_group"] + (kf // 32) * ex["loop"] + (ex["ragged"] if kf % 32 else 0))
    t = ex["tail"]
    return {"prologue": pro, "setup": ex["setup"] if kf > 0 else 0, "groups": scan, "repair_per_wavefront": groups * ex["repair"],
            "handover": ex["handover"], "compaction": comp, "outside_scan": pro + ex["handover"] + comp,
            "mfma": groups * ceil(kf, 32) * 16,
            "tail_survivor": t["lane0"], "tail_non_survivor": t["lane0"] + t["finite_count"],
            "tail_void": t["void_only"] + t["lane0"], "void_wavefront": t["entry"]}


def launch(ex, kf, kt, survivors, non_survivors, void):
    """Vector instructions of one launch (4 wavefronts per slot; MFMAs listed apart: the counter SQ_INSTS_VALU holds both).
    A survivor's wavefronts decide the second best again once per group, a non-survivor's never; lane 0's tail is counted
    whole for survivors and void slots, which run less of it (an upper bound, 0.3 % of the total at the benchmark's mix)."""
    e = executed(ex, kf, kt)
    wave = e["prologue"] + e["setup"] + e["groups"] + e["handover"] + e["compaction"]
    valu = (survivors * (4 * (wave + e["repair_per_wavefront"]) + e["tail_survivor"]) +
            non_survivors * (4 * wave + e["tail_non_survivor"]) + void * (4 * e["void_wavefront"] + e["tail_void"]))
    mfma = (survivors + non_survivors) * 4 * e["mfma"]
    return {"valu": valu, "mfma": mfma, "valu_and_mfma": valu + mfma, "per_wavefront": e}


def run(asm_path):
    lines = open(asm_path).readlines()
    rows, model, repaired, whole, ex = census(function_lines(lines, SPLIT))
    return {"regions": {k: {x: v[x] for x in KINDS} for k, v in rows.items()}, "model_valu": model,
            "model_valu_repaired": repaired,
            "kernel_total": {x: whole[x] for x in KINDS}, "executed_model": ex,
            "k_match_split<8,4,3>": resources(lines, SPLIT), "k_verify_fused<8,0,false>": resources(lines, FUSED)}


def mix_of(text):
    """--mix "Kf,Kt,survivors,non-survivors,void slots" """
    v = [int(x) for x in text.split(",")]
    if len(v) != 5 or min(v) < 0:
        sys.exit("--mix wants Kf,Kt,survivors,non_survivors,void_slots")
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--figures", help="a --json output made before: the executed model runs on its figures, nothing is compiled")
    ap.add_argument("--mix", action="append", help="Kf,Kt,survivors,non_survivors,void_slots of one launch (may repeat)")
    a = ap.parse_args()
    if a.figures:
        r = json.load(open(a.figures))
    elif a.asm:
        r = run(a.asm)
    else:
        with tempfile.TemporaryDirectory() as td:
            compile_asm(os.path.join(td, "tu.s"))
            r = run(os.path.join(td, "tu.s"))
    mixes = [mix_of(m) for m in (a.mix or [BENCH_MIX])]
    r["launches"] = [dict(zip(("kf", "kt", "survivors", "non_survivors", "void"), m), **launch(r["executed_model"], *m))
                     for m in mixes]
    if a.json:
        print(json.dumps(r))
        return
    print("k_match_split<8, 4, 3>, per wavefront  (flags: %s)" % " ".join(FLAGS[1:]))
    print("  %-82s %5s %5s %5s %5s %5s" % (("region",) + tuple(k.upper() for k in KINDS)))
    for k, v in r["regions"].items():
        print("  %-82s %5d %5d %5d %5d %5d" % ((k,) + tuple(v[x] for x in KINDS)))
    print("  %-82s %5d %5d %5d %5d %5d" % (("whole kernel (static)",) + tuple(r["kernel_total"][x] for x in KINDS)))
    for k, v in r["model_valu"].items():
        print("  modelled VALU per wavefront, K = %4d: %d  (second best decided again: %d)"
              % (int(k), v, r["model_valu_repaired"][k]))
    for name in ("k_match_split<8,4,3>", "k_verify_fused<8,0,false>"):
        print("  %-28s VGPRs %s, scratch %s B, occupancy %s" % (name, r[name]["vgprs"], r[name]["scratch_bytes"], r[name]["occupancy"]))
    ex = r["executed_model"]
    print("executed model: what the loops outside the scan cost per trip, lane 0's tail by what it holds")
    for lp in ex["prologue"]["loops"]:
        print("  prologue loop, one trip per %4d \"from\" rows: %3d VALU  (the rest of the prologue: %d)"
              % (lp["rows_per_trip"], lp["valu"], ex["prologue"]["base"]))
    c = ex["compaction"]
    print("  compaction: %d VALU always, %s" % (c["always"], "a loop of %d per 256 rows" % c["loop"] if c["loop"] else
                                                "unrolled trips of %s" % " ".join(str(x) for x in c["trips"])))
    t = ex["tail"]
    print("  lane 0's tail: %d VALU; the count of finite points %d per trip; the pose of an estimate %d (never run: the "
          "state is null); void slots only %d" % (t["lane0"], t["finite_count"], t["pose"], t["void_only"]))
    for L in r["launches"]:
        e = L["per_wavefront"]
        print("launch of %d survivors, %d non-survivors, %d void slots at Kf = %d, Kt = %d:"
              % (L["survivors"], L["non_survivors"], L["void"], L["kf"], L["kt"]))
        print("  per wavefront: prologue %d, scan set-up %d, groups %d (+ %d where the second best is decided again), hand-over "
              "%d, compaction %d; outside the scan %d; MFMA %d" % (e["prologue"], e["setup"], e["groups"],
                                                                   e["repair_per_wavefront"], e["handover"], e["compaction"],
                                                                   e["outside_scan"], e["mfma"]))
        print("  first wavefront's tail: survivor %d, non-survivor %d, void slot %d"
              % (e["tail_survivor"], e["tail_non_survivor"], e["tail_void"]))
        print("  launch: VALU %.2f M + MFMA %.2f M = %.2f M  (SQ_INSTS_VALU counts both)"
              % (L["valu"] / 1e6, L["mfma"] / 1e6, L["valu_and_mfma"] / 1e6))


if __name__ == "__main__":
    main()
