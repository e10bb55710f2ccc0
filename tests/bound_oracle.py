"""The CPU model of context-bound proofs (format kosk-bind-v1) -- tests only.

Nothing under oracle/ changes and the oracle has no hook between its commitments and its challenges, so the model is DERIVED from it at test
time: oracle/kosk_oracle.c is read as text, exactly the two call sites that hash a whole digest table,

    ko_sha3_256(h1, tcomm_all, (size_t)KO_PARTIES * 32)          derive_alpha:  prover and verifier
    ko_sha3_256(ch, digests_all, (size_t)KO_PARTIES * 32)        derive_opened: prover and verifier

are replaced by calls of ko_bound_sha3, which hashes `table || B` when a binding value has been set with ko_bound_set(const uint8_t *) and
the table alone otherwise, and the result is compiled with the compiler and the flags of oracle/Makefile into a temporary directory that
goes with the process.  The prover and the verifier of the oracle share the two sites, so one substitution covers both.  Each pattern must
occur exactly once: anything else fails loudly here, not as a wrong proof somewhere else.

B itself is computed with hashlib (bind_value below), never by the code under test.  The binding value is a global of the model: not for
concurrent use.
"""
import atexit
import ctypes as C
import functools
import hashlib
import os
import re
import shutil
import subprocess
import tempfile

from tests import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
SITES = ("ko_sha3_256(h1, tcomm_all, (size_t)KO_PARTIES * 32)", "ko_sha3_256(ch, digests_all, (size_t)KO_PARTIES * 32)")
PRELUDE = r"""
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
void ko_sha3_256(uint8_t out[32], const uint8_t *in, size_t inlen);
static uint8_t ko_bound_B[32];
static int ko_bound_on;
void ko_bound_set(const uint8_t *b)
{
    ko_bound_on = b != NULL;
    if (b) memcpy(ko_bound_B, b, 32);
}
static void ko_bound_sha3(uint8_t out[32], const uint8_t *in, size_t inlen)
{
    if (!ko_bound_on) { ko_sha3_256(out, in, inlen); return; }
    uint8_t *m = (uint8_t *)malloc(inlen + 32);
    if (!m) abort();
    memcpy(m, in, inlen);
    memcpy(m + inlen, ko_bound_B, 32);
    ko_sha3_256(out, m, inlen + 32);
    free(m);
}
"""


def bind_value(k, pk, context):
    """B = SHA3-256("kosk-bind-v1" || 00 00 00 00 || LE32(K) || SHA3-256(pk) || context), 84 bytes hashed"""
    assert len(context) == 32
    m = b"kosk-bind-v1" + bytes(4) + k.to_bytes(4, "little") + hashlib.sha3_256(pk).digest() + bytes(context)
    assert len(m) == 84
    return hashlib.sha3_256(m).digest()


def derived_source():
    with open(os.path.join(ORACLE_DIR, "kosk_oracle.c")) as f:
        src = f.read()
    for site in SITES:
        n = src.count(site)
        if n != 1:
            raise RuntimeError("bound_oracle: %r occurs %d times in oracle/kosk_oracle.c, expected exactly once" % (site, n))
        src = src.replace(site, site.replace("ko_sha3_256(", "ko_bound_sha3(", 1))
    return PRELUDE + src


def _makefile_var(text, name):
    m = re.search(r"^%s\s*\?=\s*(.*)$" % name, text, re.M)
    if not m:
        raise RuntimeError("bound_oracle: oracle/Makefile sets no " + name)
    return m.group(1).strip()


@functools.lru_cache(maxsize=None)
def model():
    """the derived model as a ctypes library (built once per process)"""
    with open(os.path.join(ORACLE_DIR, "Makefile")) as f:
        mk = f.read()
    cc, cflags = os.environ.get("CC") or _makefile_var(mk, "CC"), _makefile_var(mk, "CFLAGS").split()
    if not shutil.which(cc):
        cc = "cc"  # what make itself falls back to
    tmp = tempfile.mkdtemp(prefix="kosk_bound_oracle_")
    atexit.register(shutil.rmtree, tmp, True)
    c_path, so_path = os.path.join(tmp, "kosk_bound_oracle.c"), os.path.join(tmp, "libkosk_bound_oracle.so")
    with open(c_path, "w") as f:
        f.write(derived_source())
    r = subprocess.run([cc] + cflags + ["-I" + ORACLE_DIR, "-shared", "-o", so_path, c_path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        raise RuntimeError("bound_oracle: compiling the derived model failed\n" + r.stdout)
    lib = C.CDLL(so_path)
    lib.ko_bound_set.argtypes = [C.c_char_p]
    lib.ko_bound_set.restype = None
    lib.ko_keygen.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def keygen_pk(k, tape):
    """the public key ko_keygen makes from the first 64 bytes of the tape"""
    p = oracle_lib.params(k)
    t = oracle_lib.Tape(tape, len(tape), 0, 0, 0)
    pk, sk, raw = C.create_string_buffer(p.pk_bytes), C.create_string_buffer(p.sk_bytes), oracle_lib.Mlwe()
    model().ko_keygen(k, C.byref(t), pk, sk, C.byref(raw))
    return pk.raw


def verifiable_keygen(k, tape, context=None, bind=None):
    """ko_verifiable_keygen of the derived model -> (pk, sk, pi).  context: the proof is bound to (its own pk, context); bind: to this B as
    given; neither: no binding is set, the plain oracle's transcript"""
    lib, p = model(), oracle_lib.params(k)
    if context is not None:
        bind = bind_value(k, keygen_pk(k, tape), context)
    t = oracle_lib.Tape(tape, len(tape), 0, 0, 0)
    pk, sk, pi = C.create_string_buffer(p.pk_bytes), C.create_string_buffer(p.sk_bytes), C.create_string_buffer(p.proof_bytes)
    lib.ko_bound_set(bind)
    try:
        lib.ko_verifiable_keygen(k, C.byref(t), pk, sk, pi, None)
    finally:
        lib.ko_bound_set(None)
    assert not t.overrun
    if context is not None:
        assert bind == bind_value(k, pk.raw, context)
    return pk.raw, sk.raw, pi.raw


def verify(k, pi, pk, context=None, bind=None):
    """ko_kosk_verify of the derived model under B(pk, context), under `bind` as given, or with no binding set -> bool"""
    lib = model()
    if context is not None:
        bind = bind_value(k, pk, context)
    why = C.create_string_buffer(256)
    lib.ko_bound_set(bind)
    try:
        return bool(lib.ko_kosk_verify(k, C.c_char_p(pi), C.c_char_p(pk), why, 256))
    finally:
        lib.ko_bound_set(None)


# the pinned case of tests/golden/bound_v1.json: tape SHAKE256("kosk-tape-v1:0"), context 00 01 .. 1f
PIN_CONTEXT = bytes(range(32))


@functools.lru_cache(maxsize=None)
def pinned(k):
    """(pk, sk, bound pi) of the pinned case, computed once per process"""
    return verifiable_keygen(k, oracle_lib.tape_bytes_for(k, 0), context=PIN_CONTEXT)


@functools.lru_cache(maxsize=None)
def case(k, index, context):
    """(pk, sk, bound pi) on tape `index` under `context`, computed once per process and shared by the tests"""
    return verifiable_keygen(k, oracle_lib.tape_bytes_for(k, index), context=context)


def context_of(i):
    """test contexts: distinct, no structure the library could special-case"""
    return hashlib.sha3_256(b"kosk-bind-test-context:%d" % i).digest()
