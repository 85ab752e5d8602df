#!/usr/bin/env python3
"""Register-pressure check of the closest-point traversal kernels (CPU only, no GPU needed).

Compiles mesh_amd/csrc/nearest.hip to gfx950 assembly (optionally with extra -D flags) and reports, for k_knn_lean<MODE>,
k_knn_list<MODE, false, PF> and k_knn_queue<MODE, false> (MODE 0 and 3), the register and spill counts of the code object's metadata, and what
sits inside the tile's wave loop (found from LLVM's loop annotations as the parent of the loop with the fp64 construction): scratch (VGPR spill) instructions,
lane reads and writes (v_readlane / v_writelane: SGPR spill traffic), and the static VALU / SALU / branch counts, split
into the leaf rounds (the innermost loop that holds the fp64 construction) and the node step (the rest of the wave
loop).  A spill reload inside that loop costs a memory round trip per iteration: A/B runs showed -13 % for two such
reloads, so a variant with loop spills is not worth a GPU session.

    python scripts/isa_check.py [-DMSH_LEAF_Q=4 ...]

--save FILE only writes the assembly; --diff FILE (the --save of another tree) compares the two kernel by kernel instead
of reporting -- the .amdhsa_* block and the instruction text, comments dropped and labels renumbered -- and exits 1
when any kernel differs (for such a kernel it also says whether the register, spill, LDS and private-segment figures of
the metadata held).  Two compiles of one source differ only in the __hip_cuid_* symbol, so a refactor that should
not touch the generated code shows "identical" for every kernel.  Both take --src FILE, a source of mesh_amd/csrc to
compile (default nearest.hip; the report is of nearest.hip's kernels only), any number of times, or --src all for every
.hip file: the kernels of all of them are compared by name, so code may move between files (knn.h's users, cutbuild.hip
and sort.hip hold what nearest.hip held); a kernel renamed by a split is found through pre_split().  A tree from before
these options gets a copy of this script first (it compiles the sources beside it):

    cp scripts/isa_check.py ../parent/scripts/ && python ../parent/scripts/isa_check.py --src all --save /tmp/parent.s
    python scripts/isa_check.py --src all --diff /tmp/parent.s
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(R, "mesh_amd", "csrc")


def compile_asm(flags, src="nearest.hip"):
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950",
           "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out] + flags
    subprocess.run(cmd, check=True, cwd=CSRC, stderr=subprocess.DEVNULL)
    with open(out) as f:
        s = f.read()
    os.unlink(out)
    return s


def blocks(body):
    """(label, loops, lines) per basic block of a kernel's assembly; loops = headers of the loops that hold the
    block, outermost first (LLVM's "Parent Loop" / "This Loop Header" / "in Loop: Header=" annotations)."""
    out, cur, loops, label = [], [], [], "entry"
    chain = {}  # loop header -> its chain of headers
    lines = body.split("\n")
    for k, line in enumerate(lines):  # headers first: a block can precede its loop's header in the layout
        if line.startswith(".LBB"):
            note = [line]
            while k + 1 < len(lines) and lines[k + 1].lstrip().startswith(";") and "Loop" in lines[k + 1]:
                k += 1
                note.append(lines[k])
            note = "\n".join(note)
            if "Loop Header: Depth=" in note:
                lab = line.split(":")[0].lstrip(".L")
                chain[lab] = re.findall(r"Parent Loop (\w+) Depth=", note) + [lab]
    k = 0
    while k < len(lines):
        line = lines[k]
        if line.startswith(".LBB") or line.startswith("; %bb"):
            if cur:
                out.append((label, loops, cur))
            label, cur = line.split(":")[0].lstrip(".L"), []
            note = [line]
            while k + 1 < len(lines) and lines[k + 1].lstrip().startswith(";") and "Loop" in lines[k + 1]:
                k += 1
                note.append(lines[k])
            note = "\n".join(note)
            m = re.search(r"in Loop: Header=(\w+) Depth=", note)
            if m:
                loops = chain.get(m.group(1), [m.group(1)])
            elif "Loop Header: Depth=" in note:
                loops = re.findall(r"Parent Loop (\w+) Depth=", note) + [label]
                chain[label] = loops
            else:
                loops = []
            k += 1
            continue
        t = line.strip()
        if t and not t.startswith(";") and not t.startswith("."):
            cur.append(t)
        k += 1
    if cur:
        out.append((label, loops, cur))
    return out


def classify(ins):
    op = ins.split()[0]
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    return "mem"


LEAN0 = "_ZN3msh10k_knn_leanILi0EEEvNS_7KnnArgsE"  # the headline's pass-1 kernel


def metadata(s, name):
    """the register, spill, LDS and private-segment figures of the kernel with mangled name `name`, from the code
    object's metadata"""
    at = re.search(r"\.name:\s+" + name + r"\n", s).start()
    # the metadata lists a kernel's keys in alphabetical order around .name
    meta, head = s[at:][:1500], s[:at][-600:]

    def md(key, text):
        m = re.findall(r"\." + key + r":\s+(\d+)", text)
        return int(m[-1] if text is head else m[0]) if m else None

    r = {}
    for key in ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size"):
        r[key] = md(key, meta)
    r["group_segment_fixed_size"] = md("group_segment_fixed_size", head)
    return r


def report(s, name, tag):
    """the record of the kernel with mangled name `name`, led by the caller's tag (which kernel it is)"""
    r = dict(tag)
    r.update(metadata(s, name))
    # the names bench.py reads from profiles/pmc_traffic.json's isa record (waves_per_simd)
    r["vgpr"], r["vgpr_spill"], r["lds"] = r["vgpr_count"], r["vgpr_spill_count"], r["group_segment_fixed_size"]
    a = s.index(name + ":")
    b = s.index(".end_amdhsa_kernel", a)
    bl = blocks(s[a:b])
    f64 = {}  # fp64 arithmetic per innermost loop: the leaf rounds hold the exact construction
    for _, lp, ls in bl:
        if len(lp) >= 2:
            f64[lp[-1]] = f64.get(lp[-1], 0) + sum(1 for i in ls if re.match(r"v_(fma|mul|add)_f64", i))
    leaf = max(f64, key=f64.get)
    wave = next(lp for _, lp, _ in bl if lp and lp[-1] == leaf)[-2]  # the wave loop: the leaf rounds' parent
    inwave = [(lp, ls) for _, lp, ls in bl if wave in lp]
    r["scratch_ops"] = sum(1 for _, _, ls in bl for i in ls if "scratch_" in i)
    r["scratch_in_loop"] = sum(1 for _, ls in inwave for i in ls if "scratch_" in i)
    r["lane_rw_in_loop"] = sum(1 for _, ls in inwave for i in ls
                               if i.startswith("v_readlane") or i.startswith("v_writelane"))
    r["asm_lines"] = sum(len(ls) for _, _, ls in bl)
    parts = {"leaf_round": {}, "node_step": {}}
    for lp, ls in inwave:
        c = parts["leaf_round" if leaf in lp else "node_step"]
        for i in ls:
            k = classify(i)
            c[k] = c.get(k, 0) + 1
            if i.startswith("s_cbranch_execz"):
                c["execz"] = c.get("execz", 0) + 1
            if i.startswith("s_waitcnt"):
                c["waitcnt"] = c.get("waitcnt", 0) + 1
            if i.startswith("s_nop"):
                c["nop"] = c.get("nop", 0) + 1
    r.update(parts)
    return r


def kernels(s):
    """name -> normalised text of each kernel (its instructions and its .amdhsa_* block): comments dropped, the
    kernel's own name and the .LBB labels (numbered by function and block) replaced by their order of appearance."""
    out = {}
    for name in re.findall(r"^\t\.amdhsa_kernel (\S+)$", s, re.M):
        a = s.index("\n" + name + ":")
        body = s[a:s.index(".end_amdhsa_kernel", a)].replace(name, "KERNEL")
        lines = [t for t in (ln.split(";")[0].rstrip() for ln in body.split("\n")) if t.strip()]
        labels = {}

        def renumber(m):
            return labels.setdefault(m.group(0), f".L{len(labels)}")
        out[name] = [re.sub(r"\.L(?:BB|func_end)\d+(?:_\d+)?", renumber, t) for t in lines]
    return out


def pre_split(name):
    """A pass-1 kernel of an assembly from before k_knn was split, under the name it has now: k_knn<MODE, STATS, LIST, PF,
    LEAN> (before k_knn_lean was a kernel of its own) and k_knn<MODE, STATS, LIST, PF> (before the list and the queue
    path were); and the triangle walks from before k_tritri became a mode of k_tritri_all<kMode> (any hit 0, count 1,
    fill 2; they were k_tritri and k_tritri_all<kFill>)"""
    tri = {"_ZN3msh8k_tritriENS_7TriArgsE": 0, "_ZN3msh12k_tritri_allILb0EEEvNS_8PairArgsE": 1,
           "_ZN3msh12k_tritri_allILb1EEEvNS_8PairArgsE": 2}
    if name in tri:
        return f"_ZN3msh12k_tritri_allILi{tri[name]}EEEvNS_8PairArgsE"
    m = re.fullmatch(r"_ZN3msh5k_knnILi(\d)ELb(\d)ELb(\d)ELb(\d)(?:ELb(\d))?EEEvNS_7KnnArgsE", name)
    if not m:
        return name
    mode, stats, lst, pf, lean = m.groups()
    if lean == "1":
        return f"_ZN3msh10k_knn_leanILi{mode}EEEvNS_7KnnArgsE"
    if lst == "1":
        return f"_ZN3msh10k_knn_listILi{mode}ELb{stats}ELb{pf}EEEvNS_7KnnArgsE"
    return f"_ZN3msh11k_knn_queueILi{mode}ELb{stats}EEEvNS_7KnnArgsE"


def diff(s, other):
    """Compare every kernel of this tree's assembly with the one saved by --save from another tree; 1 if any differs."""
    new = kernels(s)
    with open(other) as f:
        olds = f.read()
    was = {pre_split(k): k for k in kernels(olds)}  # the name each kernel has in the other tree
    old = {pre_split(k): v for k, v in kernels(olds).items()}
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            what = "only in " + (other if name in old else "this tree")
        elif old[name] == new[name]:
            what = "identical"
        else:
            a, b = old[name], new[name]
            k = next((j for j, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            what = f"DIFFERS: {len(a)} -> {len(b)} lines, first at line {k}"
            # a refactor may change a kernel's text but not what it occupies: say whether the metadata held
            ma, mb = metadata(olds, was[name]), metadata(s, name)
            what += "; metadata " + ("kept " + str(mb) if ma == mb else f"CHANGED {ma} -> {mb}")
        bad += what != "identical"
        print(f"{what:12s} {name}")
    print(f"{len(new)} kernels, {bad} not identical")
    return 1 if bad else 0


def main():
    flags = sys.argv[1:]
    save = other = None
    srcs = []
    while "--src" in flags:  # with --save / --diff: other sources of mesh_amd/csrc, or `all` for every .hip
        srcs.append(os.path.basename(flags.pop(flags.index("--src") + 1)))
        flags.remove("--src")
    if srcs and srcs != ["nearest.hip"] and "--save" not in flags and "--diff" not in flags:
        sys.exit("--src goes with --save or --diff: the report is of nearest.hip's kernels")
    if "all" in srcs:
        srcs = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    srcs = srcs or ["nearest.hip"]
    if "--save" in flags:  # keep the assembly, for another tree's --diff
        save = flags.pop(flags.index("--save") + 1)
        flags.remove("--save")
    if "--diff" in flags:
        other = flags.pop(flags.index("--diff") + 1)
        flags.remove("--diff")
    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:  # kernel names are unique across the library
        s = "\n".join(ex.map(lambda f: compile_asm(flags, f), srcs))
    if save:
        with open(save, "w") as f:
            f.write(s)
        if not other:
            return
    if other:
        sys.exit(diff(s, other))
    for mode in (0, 3):
        print(report(s, f"_ZN3msh10k_knn_leanILi{mode}EEEvNS_7KnnArgsE", dict(kernel="k_knn_lean", mode=mode)))
    for pf in (True, False):
        for mode in (0, 3):
            print(report(s, f"_ZN3msh10k_knn_listILi{mode}ELb0ELb{int(pf)}EEEvNS_7KnnArgsE",
                         dict(kernel="k_knn_list", mode=mode, prefetch=pf)))
    for mode in (0, 3):
        print(report(s, f"_ZN3msh11k_knn_queueILi{mode}ELb0EEEvNS_7KnnArgsE", dict(kernel="k_knn_queue", mode=mode)))


if __name__ == "__main__":
    main()
