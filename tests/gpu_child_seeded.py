"""Seeded proving (format kosk-seedtape-v1): helpers of tests/test_gpu_13_seeded.py and the bodies of its cases that run in a FRESH
child Python process (tests/conftest.py: run_gpu_child) -- several handles and caller threads at once, or a handle created under a
debug variable.

    python -c "from tests.gpu_child_seeded import seeded_cohorts; seeded_cohorts(0)"
"""
import hashlib
import os
import struct

LABEL = b"kosk-seedtape-v1"
TAPE_BYTES = {2: 65280, 3: 68062, 4: 75676}


def seed_for(k, i, tag="seeded"):
    """test seed number i of parameter set k (any 32 bytes would do: sha256 of a label)"""
    return hashlib.sha256(("%s:%d:%d" % (tag, k, i)).encode()).digest()


def hashlib_tape(k, seed):
    """the normative definition of the format, with hashlib only"""
    t = TAPE_BYTES[k]
    nb = -(-t // 136)
    return b"".join(hashlib.shake_256(seed + LABEL + struct.pack("<II", k, j)).digest(136) for j in range(nb))[:t]


def device_rows(torch, rows, stride):
    """byte strings -> a device buffer with row b at b * stride (zeros between), synchronised; returns the tensor (keep it alive)"""
    import numpy as np
    host = np.zeros((len(rows), stride), np.uint8)
    for b, x in enumerate(rows):
        host[b, :len(x)] = np.frombuffer(x, np.uint8)
    dev = torch.from_numpy(host).to("cuda")
    torch.cuda.synchronize()
    return dev


def _kosk_env(k, max_batch, env, **opts):
    from mpcith_kyber_kosk_amd import api
    old = {name: os.environ.get(name) for name in env}
    os.environ.update({name: str(v) for name, v in env.items()})
    try:
        return api.Kosk(kyber_k=k, max_batch=max_batch, **opts)
    finally:
        for name, v in old.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v


def seeded_cohorts(fs, all_seeded=False, k=3, per=46, threads=6, rounds=2):
    """Six caller threads, one handle each, combine = 6: merged runs whose members bring their randomness in different ways -- seeds
    (one of them a short batch of 17), device tapes, host tapes -- or, with all_seeded, seeds only.  Every member must get exactly the
    bytes of its unmerged call (and of the explicit-tape call on the hashlib tape), and kosk_combine_stats must show merged runs."""
    import threading
    import torch
    from mpcith_kyber_kosk_amd import api
    from tests import oracle_lib as oracle
    kinds = ["seed"] * threads if all_seeded else ["seed", "dev", "host", "seed", "dev", "seed"]
    size = [per] * threads
    if not all_seeded:
        size[threads - 1] = 17  # ragged: the last member of the cohort (a short block can only end a run)
    plain = api.Kosk(kyber_k=k, max_batch=per, fs_mode=fs)
    hs = [api.Kosk(kyber_k=k, max_batch=per, combine=threads, combine_wait_us=200000, combine_idle_us=100000, fs_mode=fs) for _ in range(threads)]
    stride = (plain.tape_bytes + 63) // 64 * 64
    seeds, tapes, want = {}, {}, {}
    for t in range(threads):
        for r in range(rounds):
            sd = [seed_for(k, (t * rounds + r) * per + b, "cohort%d%d" % (fs, all_seeded)) for b in range(size[t])]
            tp = [hashlib_tape(k, s) for s in sd]
            seeds[t, r], tapes[t, r] = sd, tp
            n = size[t]
            plain.verifiable_keygen_resident(tp)  # the explicit-tape call
            pk, sk = plain.keys(n)
            pis = plain.fetch_proofs(n)
            if kinds[t] == "seed":  # the member's own unmerged call
                plain.verifiable_keygen_resident(seeds=sd)
                assert plain.keys(n) == (pk, sk) and plain.fetch_proofs(n) == pis, ("unmerged seeded call differs from the explicit one", t, r)
            assert plain.verify_resident_pk(n) == [True] * n
            want[t, r] = (pk, sk, pis)
    for (t, r, b) in ((0, 0, 0), (threads - 1, rounds - 1, size[threads - 1] - 1)):
        opk, osk, opi, _, _ = oracle.verifiable_keygen(k, tapes[t, r][b])
        assert (want[t, r][0][b], want[t, r][1][b], want[t, r][2][b]) == (opk, osk, opi)
    errs = []
    barrier = threading.Barrier(threads)
    base = [None] * threads

    def call(h, t, r):
        n = size[t]
        if kinds[t] == "seed":
            h.verifiable_keygen_resident(seeds=seeds[t, r])
        elif kinds[t] == "host":
            h.verifiable_keygen_resident(tapes[t, r])
        else:
            dev = device_rows(torch, tapes[t, r], stride)
            h.verifiable_keygen_resident(dev.data_ptr(), n=n, tape_stride=stride)
            del dev
        return n

    def worker(t):
        try:
            h = hs[t]
            barrier.wait()
            for _ in range(2):  # nobody is expected at a cohort's very first call: two unchecked rounds bring the callers into step
                n = call(h, t, 0)
                assert h.verify_resident_pk(n) == [True] * n
            base[t] = h.combine_stats()
            for r in range(rounds):
                n = call(h, t, r)
                assert h.keys(n) == want[t, r][:2], ("keys", t, r)
                assert h.verify_resident_pk(n) == [True] * n and h.fail_masks(n) == [0] * n, ("verify", t, r)
                assert h.fetch_proofs(n) == want[t, r][2], ("proofs", t, r)
        except Exception as e:  # noqa: BLE001
            errs.append((t, repr(e)))
            try:
                barrier.abort()
            except Exception:
                pass
    ths = [threading.Thread(target=worker, args=(t,)) for t in range(threads)]
    for x in ths:
        x.start()
    for x in ths:
        x.join()
    assert not errs, errs
    calls = sum(h.combine_stats()[0] - base[t][0] for t, h in enumerate(hs))
    members = sum(h.combine_stats()[1] - base[t][1] for t, h in enumerate(hs))
    assert calls == threads * 2 * rounds, (calls, members)
    assert members > calls, ("no call was merged", calls, members)
    launches = sum(h.path_counts()["tape_expand"] for h in hs)
    nseeded = sum(1 for x in kinds if x == "seed") * (2 + rounds)
    assert 0 < launches <= nseeded
    if all_seeded:  # one staging copy and one expansion launch per run: merged runs make fewer launches than there were calls
        assert launches < nseeded, (launches, nseeded)
    for h in hs + [plain]:
        h.close()
    print("seeded_cohorts ok fs %d all_seeded %d mean callers per run %.2f expansion launches %d for %d seeded calls"
          % (fs, all_seeded, members / calls, launches, nseeded))


def seeded_graph_replay(k=3, n=3):
    """KOSK_GRAPHS=1: seeded calls, device tapes and host tapes alternating on one handle whose segments are captured and replayed;
    the expansion launch stays outside the captured segments.  Same bytes as the plain-launch handle."""
    import torch
    from mpcith_kyber_kosk_amd import api
    from tests import oracle_lib as oracle
    seeds = [seed_for(k, i, "graph") for i in range(n)]
    other = [seed_for(k, i, "graph-b") for i in range(n)]
    tapes, tapes_b = [hashlib_tape(k, s) for s in seeds], [hashlib_tape(k, s) for s in other]
    plain = api.Kosk(kyber_k=k, max_batch=n)
    want, want_b = plain.verifiable_keygen(tapes), plain.verifiable_keygen(tapes_b)
    assert want[2][0] == oracle.verifiable_keygen(k, tapes[0])[2]
    g = _kosk_env(k, n, {"KOSK_GRAPHS": "1"})
    stride = (g.tape_bytes + 63) // 64 * 64
    dev_b = device_rows(torch, tapes_b, stride)
    for rep in range(3):  # first calls capture, later calls replay
        assert g.verifiable_keygen(seeds=seeds) == want, ("seeded batch", rep)
        g.verifiable_keygen_resident(dev_b.data_ptr(), n=n, tape_stride=stride)  # device tapes read in place
        assert g.keys(n) == want_b[:2] and g.fetch_proofs(n) == want_b[2], ("device tapes", rep)
        g.stage_prover_inputs(seeds=seeds)  # the staged form: prove_resident's first segment is a captured graph keyed by the tape buffer
        g.prove_resident(n)
        assert g.keys(n) == want[:2] and g.fetch_proofs(n) == want[2], ("seeded staged", rep)
        assert g.verifiable_keygen(tapes_b) == want_b, ("host tapes", rep)
        g.stage_prover_inputs(seeds=other)
        g.prove_resident(n)
        assert g.keys(n) == want_b[:2] and g.fetch_proofs(n) == want_b[2], ("seeded staged, other seeds", rep)
        g.stage_prover_inputs(tapes)
        g.prove_resident(n)
        assert g.fetch_proofs(n) == want[2], ("host tapes staged", rep)
        g.verifiable_keygen_resident(seeds=other[:2])  # another batch size
        assert g.fetch_proofs(2) == want_b[2][:2], ("seeded resident", rep)
    pc = g.path_counts()
    assert pc["graph_replay"] > 0 and pc["tape_expand"] == 3 * 4
    assert g.verify(want[2], want[0]) == [True] * n
    g.close()
    plain.close()
    print("seeded_graph_replay ok", k, pc["graph_replay"])
