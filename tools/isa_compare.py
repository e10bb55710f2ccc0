#!/usr/bin/env python3
"""Compare the kernels of two gfx950 assembly listings, kernel by kernel: histogram of instruction mnemonics, num_vgpr, num_agpr,
private_seg_size and .amdhsa_group_segment_fixed_size.

    hipcc -O3 -std=c++20 --offload-arch=gfx950 -x hip --cuda-device-only -S <tree>/mpcith_kyber_kosk_amd/csrc/kosk_kernels.hip -o <tree>.s
    python tools/isa_compare.py old.s new.s

Exit status 1 if a kernel of both listings grew in any mnemonic or in num_vgpr."""
import collections
import re
import subprocess
import sys

RES = ("num_vgpr", "num_agpr", "private_seg_size")


def kernels(path):
    text = open(path).read()
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M):
        body = text[text.index("\n%s:" % name):]
        body = body[:body.index("\n.Lfunc_end")]
        hist = collections.Counter(m for m in re.findall(r"^\t([a-z]\w*)", body, re.M))
        res = {r: int(re.search(r"\.set %s\.%s, (\d+)" % (re.escape(name), r), text).group(1)) for r in RES}
        desc = text[text.index(".amdhsa_kernel %s\n" % name):]
        res["lds"] = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
        out[name] = (hist, res)
    # keyed by the demangled name without a template argument a later tree dropped (k_fs_chain<M, FsSpongeBperm> is k_fs_chain<M>,
    # k_table_gemm<13, 1, 3> is k_table_gemm<13, 3>)
    pretty = subprocess.run(["c++filt", "-p"] + list(out), capture_output=True, text=True).stdout.split("\n")
    return {re.sub(r", kosk::FsSpongeBperm>", ">", p).replace("k_table_gemm<13, 1, 3>", "k_table_gemm<13, 3>"): v for p, v in zip(pretty, out.values())}


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    names = sorted(set(old) | set(new))
    print("kernels: %d old, %d new" % (len(old), len(new)))
    grew = False
    for n in names:
        if n not in old or n not in new:
            print("%-8s %s" % ("removed" if n in old else "added", n))
            continue
        (ho, ro), (hn, rn) = old[n], new[n]
        diff = {m: hn[m] - ho[m] for m in set(ho) | set(hn) if hn[m] != ho[m]}
        rdiff = {r: (ro[r], rn[r]) for r in ro if ro[r] != rn[r]}
        grew |= any(d > 0 for d in diff.values()) or rn["num_vgpr"] > ro["num_vgpr"]
        print("%-8s %s  %d instructions, vgpr %d agpr %d scratch %d lds %d" % ("changed" if diff or rdiff else "same", n, sum(hn.values()), *rn.values()))
        if diff or rdiff:
            print("         mnemonics (new - old): %s  resources (old, new): %s" % (dict(sorted(diff.items())), rdiff))
    return 1 if grew else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
