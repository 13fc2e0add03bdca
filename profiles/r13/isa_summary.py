"""The memory-event sequence and the resource table of sp_fused_kernel from its gfx950 assembly:

    hipcc -O3 --offload-arch=gfx950 -fPIC -std=c++17 -S --cuda-device-only admm_net_amd/csrc/spectral_fused.hip -o sf.s
    python profiles/r13/isa_summary.py sf.s                 # the resource table of the six instantiations
    python profiles/r13/isa_summary.py sf.s 3 12            # + the event sequence of sp_fused_kernel<3, 12>
    python profiles/r13/isa_summary.py sf.s 3 12 --loops    # the sequence cut down to the bodies of its loops

An event is a vector-memory instruction (global / scratch load or store), an `s_waitcnt` with a vmcnt field, a barrier, an MFMA
run (collapsed to its length), a label or a branch.  Loads and stores in a row are collapsed to `N x name`.  `vmcnt(N)` waits until
at most N vector-memory operations are outstanding: N = 0 in front of arithmetic means that nothing is in flight behind it.
"""
import re
import sys

EVENT = re.compile(r"^\s+(global_load\w*|global_store\w*|global_atomic\w*|scratch_load\w*|scratch_store\w*|s_barrier|"
                   r"s_cbranch_\w+|s_branch|v_mfma\w*|s_waitcnt)\b(.*)$")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size",
        "max_flat_workgroup_size")


def kernels(text):
    """{(TPW, W): (body lines, metadata dict)} of the sp_fused_kernel instantiations in an assembly file."""
    out = {}
    lines = text.splitlines()
    starts = [(i, m) for i, l in enumerate(lines)
              for m in [re.match(r"^(_ZN7admmnet15sp_fused_kernelILi(\d+)ELi(\d+)EE\w+):", l)] if m]
    for i, m in starts:
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        out[(int(m.group(2)), int(m.group(3)))] = [lines[i:end], {}, m.group(1)]
    # amdhsa.kernels: one block per kernel, opened by "  - .key:", its keys in alphabetical order around .name
    blocks, cur = [], None
    for l in lines:
        if re.match(r"^  - \.\w+:", l):
            cur = {}
            blocks.append(cur)
        m = re.match(r"^\s+(?:- )?\.(\w+):\s+(\S+)\s*$", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    for blk in blocks:
        for k in out.values():
            if k[2] == blk.get("name"):
                k[1].update({key: int(blk[key]) for key in META if key in blk})
    return out


def occupancy(meta):
    """Waves per SIMD by registers (512 per lane per SIMD, allocated in blocks of 8; AGPRs share the file) and the workgroups
    per CU that leaves for this workgroup size."""
    regs = (meta["vgpr_count"] + meta.get("agpr_count", 0) + 7) // 8 * 8
    waves = min(8, 512 // regs)
    per_simd = meta["max_flat_workgroup_size"] // 64 // 4 or 1
    return waves, waves // per_simd


def events(body):
    ev = []
    for l in body:
        m = LABEL.match(l)
        if m:
            ev.append(("label", m.group(1)))
            continue
        m = EVENT.match(l)
        if not m:
            continue
        op, rest = m.group(1), m.group(2)
        if op == "s_waitcnt":
            v = re.search(r"vmcnt\((\d+)\)", rest)
            if v:
                ev.append(("wait", "vmcnt(%s)" % v.group(1)))
        elif op.startswith("s_cbranch") or op == "s_branch":
            ev.append(("branch", "%s %s" % (op, rest.strip())))
        else:
            ev.append(("mem" if not op.startswith(("s_barrier", "v_mfma")) else "op", op))
    return ev


def collapse(ev):
    out = []
    for kind, what in ev:
        if out and kind in ("mem", "op") and out[-1][0] == kind and out[-1][1] == what:
            out[-1][2] += 1
        else:
            out.append([kind, what, 1])
    return out


def loops(ev):
    """[(first, last)] index ranges of the innermost backward branches."""
    pos = {what: i for i, (kind, what) in enumerate(ev) if kind == "label"}
    spans = []
    for i, (kind, what) in enumerate(ev):
        if kind == "branch":
            tgt = what.split()[-1]
            if tgt in pos and pos[tgt] < i:
                spans.append((pos[tgt], i))
    return [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]


def show(ev):
    for kind, what, cnt in collapse(ev):
        if kind == "label":
            print("%s:" % what)
        elif kind == "branch":
            print("      %s" % what)
        else:
            print("    %s%s" % ("%d x " % cnt if cnt > 1 else "", what))


def main():
    text = open(sys.argv[1]).read()
    ks = kernels(text)
    print("| kernel | VGPRs | spilled | scratch bytes | static LDS | waves / SIMD | workgroups / CU |")
    print("|---|---|---|---|---|---|---|")
    for key in sorted(ks, key=lambda k: (k[1], k[0])):
        meta = ks[key][1]
        w, g = occupancy(meta)
        print("| `<%d, %d>` | %d | %d | %d | %d | %d | %d |" % (key[0], key[1], meta["vgpr_count"], meta["vgpr_spill_count"],
                                                               meta["private_segment_fixed_size"], meta["group_segment_fixed_size"], w, g))
    if len(sys.argv) >= 4:
        ev = events(ks[(int(sys.argv[2]), int(sys.argv[3]))][0])
        if "--loops" in sys.argv:
            for a, b in loops(ev):
                print("-- loop %s" % ev[a][1])
                show(ev[a:b + 1])
        else:
            show(ev)


if __name__ == "__main__":
    main()
