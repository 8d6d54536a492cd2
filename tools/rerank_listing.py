"""dev: the two static figures of the merged-record re-rank, read from the device listing of search.hip (no GPU needed):

    hipcc $(make -s -C text2loc_amd/csrc print-flags) -S --cuda-device-only text2loc_amd/csrc/search.hip -o search.s
    python tools/rerank_listing.py search.s

Per instance rerank_kernel<8, 16, true, FORM>: registers and spills; the VALU / s_nop count of the twelve up-front merge rounds (from
the first DPP maximum behind the record loads to the last select of the twelfth round: the first ds_bpermute of the row exchange ends
it); and where the twelve early global_load_dwordx4 of database rows stand relative to the first s_waitcnt vmcnt that waits for one of them."""
import re
import sys


def body(lines, sym):
    i = next(k for k, l in enumerate(lines) if l.startswith(sym + ":"))
    j = next(k for k in range(i, len(lines)) if lines[k].strip().startswith("s_endpgm"))
    return [l.strip() for l in lines[i + 1:j + 1]]


def is_inst(l):
    return bool(l) and not l.startswith((";", ".", "//")) and not l.endswith(":")


def main(path):
    lines = open(path).read().split("\n")
    stripped = [l.strip() for l in lines]
    syms = sorted({m.group(1) for l in lines for m in [re.match(r"^(_Z\w*rerank_kernelILi8ELi16ELb1E\w*):", l)] if m})
    for sym in syms:
        b = [re.sub(r"\s*;.*$", "", l) for l in body(stripped, sym)]
        b = [l for l in b if is_inst(l)]
        meta = {}
        # metadata block of this kernel: the .vgpr_count lines follow its .symbol line
        for idx, l in enumerate(stripped):
            if l.startswith(".symbol:") and sym + ".kd" in l:
                for m in stripped[idx:idx + 12]:
                    if m.startswith((".vgpr_count", ".vgpr_spill_count")):
                        meta[m.split(":")[0]] = int(m.split(":")[1])
        print(sym)
        print("  ", meta)
        # a merge round begins at the first DPP step of its maximum (with the s_nop in front) and ends where the next round's begins;
        # the first such maximum of the kernel is floor_max, the next twelve are the up-front rounds. The twelfth round's end is not
        # marked in the listing (what follows is scheduled into it): rounds 1..11 are counted and the mean stands in for the twelfth.
        first = [i for i, l in enumerate(b) if l.startswith("v_max_f32_dpp") and "quad_perm:[1,0,3,2]" in l]
        bperm = [i for i, l in enumerate(b) if l.startswith("ds_bpermute")]
        end = next(i for i in bperm if i > first[12])
        per = []
        for r in range(1, 12):
            seg = b[first[r] - 1:first[r + 1] - 1]
            per.append((sum(1 for l in seg if l.startswith("v_")), sum(1 for l in seg if l.startswith("s_nop")),
                        sum(1 for l in seg if l.startswith("s_") and not l.startswith(("s_nop", "s_waitcnt")))))
        tot = [sum(x[k] for x in per) for k in range(3)]
        print("   merge rounds 1..11 as listed (VALU, s_nop, other SALU): " + " ".join("%d/%d/%d" % x for x in per))
        print("   twelve rounds (11 counted + their mean): %d VALU, %d s_nop, %d other SALU" % tuple(round(t * 12 / 11) for t in tot))
        loads = [i for i, l in enumerate(b) if l.startswith("global_load_dwordx4") and i > end]
        early = loads[:12]
        # a wait depends on a row load when its count is below the number of loads issued since the first row load (loads retire in order)
        def vm(i):
            return int(re.search(r"vmcnt\((\d+)\)", b[i]).group(1))
        issued, first_wait = 0, None
        for i in range(early[0], len(b)):
            if b[i].startswith("global_load"):
                issued += 1
            elif b[i].startswith("s_waitcnt") and "vmcnt" in b[i] and vm(i) < issued:
                first_wait = i
                break
        before = sum(1 for i in early if i < first_wait)
        print("   early row loads: %d of 12 issued before the first s_waitcnt vmcnt that waits for one of them (%s)" % (before, b[first_wait]))
        print("   order from the first row load: " + " ".join("L" if b[i].startswith("global_load") else "W(%s)" % re.search(r"vmcnt\((\d+)\)", b[i]).group(1)
                                                     for i in range(early[0], early[-1] + 40) if b[i].startswith("global_load_dwordx4") or (b[i].startswith("s_waitcnt") and "vmcnt" in b[i]))[:400])


if __name__ == "__main__":
    main(sys.argv[1])
