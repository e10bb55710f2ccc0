"""Writes tests/golden/seedtape_v1.json: anchors of the seeded-proving tape format kosk-seedtape-v1 (include/kosk_mi355x.h),
computed with hashlib only -- nothing of the library under test takes part.

    python tests/golden/make_seedtape_vectors.py

For Kyber parameter K and a 32-byte seed, with T = kosk_tape_bytes(K) and NB = ceil(T / 136):
    block_j = SHAKE256(seed || "kosk-seedtape-v1" || LE32(K) || LE32(j))[0:136]     j = 0 .. NB - 1
    tape    = (block_0 || block_1 || ... || block_{NB-1})[0:T]
"""
import hashlib
import json
import os
import struct

LABEL = b"kosk-seedtape-v1"
RATE = 136


def tape_bytes(k):
    """64 + 32 M + 302 nfresh (csrc/kosk_params.hpp): 65 280 / 68 062 / 75 676"""
    eta1 = 3 if k == 2 else 2
    m = 70 + 2 * k + 1
    e, z = 2 * eta1 + 1, 2 * eta1
    nfresh = 2 * m + 2 * k * e + 2 * k + k + 2 * k * z
    return 64 + 32 * m + 302 * nfresh


def tape_from_seed(k, seed):
    assert len(seed) == 32 and len(LABEL) == 16
    t = tape_bytes(k)
    nb = -(-t // RATE)
    return b"".join(hashlib.shake_256(seed + LABEL + struct.pack("<II", k, j)).digest(RATE) for j in range(nb))[:t]


def main():
    seed = bytes(range(32))
    out = {"format": "kosk-seedtape-v1", "seed": seed.hex(), "anchors": {}}
    for k in (2, 3, 4):
        tape = tape_from_seed(k, seed)
        out["anchors"]["k%d" % k] = {"tape_bytes": len(tape), "blocks": -(-len(tape) // RATE), "sha3_256": hashlib.sha3_256(tape).hexdigest(),
                                     "head": tape[:8].hex(), "tail": tape[-4:].hex()}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "seedtape_v1.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    main()
