"""The buffer inventory (csrc/kosk_inventory.hpp) without a GPU: tests/inventory_host_check.cpp is a stand-alone program on
counting malloc / free, built with ASan + UBSan and run as a child process.  It asserts, with its own counters: release(group) frees exactly
that group; an allocation that fails at any position of a group leaves, after the caller's release(group), no entry, null pointers and as
many frees as allocations, and the retry gives the entries of a first try; a view lists the arena's per-proof entries shifted by `first`
strides, owns none of them and frees only what it allocated itself; aliases are never freed; adopt + release; and the secret regions of an
owner (max_batch records) and of a view (own_batch records) are the arithmetic of kosk_wipe.hip, byte for byte."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_inventory_host_check(tmp_path):
    exe = str(tmp_path / "inventory_host_check")
    r = subprocess.run(["c++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "mpcith_kyber_kosk_amd", "csrc"), os.path.join(ROOT, "tests", "inventory_host_check.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    m = re.search(r"inventory checks (\d+) failures 0\n", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) >= 80 and "FAILED" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]


def test_the_header_is_plain_cxx():
    """no HIP in the header, and no buffer of the library is allocated or freed outside it: what is left are the caller's own
    allocations (kosk_host_alloc / kosk_host_free) and temporaries that a function frees before it returns"""
    csrc = os.path.join(ROOT, "mpcith_kyber_kosk_amd", "csrc")
    hdr = open(os.path.join(csrc, "kosk_inventory.hpp")).read()
    assert not re.search(r"#include\s*[<\"]hip|\bhip[A-Z_]\w*", hdr)
    for name in os.listdir(csrc):
        text = open(os.path.join(csrc, name)).read()
        assert "reg_buf(" not in text and "reg_pp(" not in text and "inv_drop(" not in text, name
        calls = len(re.findall(r"\bhip(?:Host)?(?:Malloc|Free)\(", text))
        assert calls == {"kosk_ctx.cpp": 6, "kosk_capi.cpp": 8}.get(name, 0), (name, calls)
