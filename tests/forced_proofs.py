"""The oracle's proofs at the forced lists of tests/opened_sets.py, made once per process and never changed: what the verifier tests at
forced opened sets verify and what the forcing GPU prover has to reproduce byte for byte.  The oracle's hook is process-wide, so the
proofs are made one after the other."""
import functools

from tests import opened_sets as osets
from tests import oracle_lib

FEW = ("first150", "run100_249", "mid600_749")  # the catalogue lists that also run at K = 2 and K = 4
HONEST_TAPE = 2100


def tape_index(k, name):
    """the tape a case is proven on: the catalogue's on 2101.. in the order the verifier tests have always used (K = 3: the catalogue's
    order; K = 2 and 4: FEW's), the candidate cases on 2150.."""
    if name in osets.CANDIDATES:
        return 2150 + list(osets.CANDIDATES).index(name)
    if k != 3 and name in FEW:
        return 2101 + FEW.index(name)
    return 2101 + list(osets.CATALOGUE).index(name)


def candidates(name):
    return osets.CANDIDATES[name] if name in osets.CANDIDATES else osets.CATALOGUE[name]


def tape(k, name):
    return oracle_lib.tape_bytes_for(k, tape_index(k, name))


@functools.lru_cache(maxsize=None)
def forced(k, name):
    """(pk, sk, pi) of the oracle's forcing prover on the case's tape, opening probe(candidates)"""
    return oracle_lib.forced_verifiable_keygen(k, tape(k, name), osets.probe(candidates(name)))


@functools.lru_cache(maxsize=None)
def honest(k, index=HONEST_TAPE):
    """(pk, sk, pi) of the oracle's own prover on tape `index`"""
    return oracle_lib.verifiable_keygen(k, oracle_lib.tape_bytes_for(k, index))[:3]
