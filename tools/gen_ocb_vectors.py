#!/usr/bin/env python3
"""AES-OCB3 through the machine's libcrypto (EVP_aes_{128,192,256}_ocb), and
the generator of tests/golden/ocb_vectors.json: the inputs follow RFC 7253
Appendix A (K = 00 01 02 .., N = BBAA99887766554433221100 + case, A and P the
bytes 00 01 02 .. of 0, 8, 16, 24, 32 or 40 bytes in the RFC's combinations),
extended to the three key sizes and to nonce lengths 1, 8, 15 and tag lengths
8, 12, 16; every output comes from libcrypto, never from this project's code.

    python tools/gen_ocb_vectors.py            # rewrite the golden file
    python tools/gen_ocb_vectors.py --check    # compare it with a fresh run

tests/test_ocb_cpu.py loads ``libcrypto_ocb`` from here for its live check."""
import argparse
import ctypes
import ctypes.util
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ocb_vectors.json")
EVP_CTRL_AEAD_SET_IVLEN, EVP_CTRL_AEAD_GET_TAG, EVP_CTRL_AEAD_SET_TAG = 0x9, 0x10, 0x11
# (AAD bytes, plaintext bytes) of the sixteen sample results of RFC 7253 Appendix A
RFC_LENGTHS = [(0, 0), (8, 8), (8, 0), (0, 8), (16, 16), (16, 0), (0, 16), (24, 24), (24, 0), (0, 24), (32, 32), (32, 0),
               (0, 32), (40, 40), (40, 0), (0, 40)]


def load_libcrypto():
    """libcrypto with the OCB ciphers, or None."""
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        lib = ctypes.CDLL(name)
        vp, cp, ip = ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)
        for f in ("EVP_CIPHER_CTX_new", "EVP_aes_128_ocb", "EVP_aes_192_ocb", "EVP_aes_256_ocb"):
            getattr(lib, f).restype = vp
        lib.EVP_CIPHER_CTX_free.argtypes = [vp]
        lib.EVP_CIPHER_CTX_ctrl.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
        lib.EVP_EncryptInit_ex.argtypes = [vp] * 3 + [cp, cp]
        lib.EVP_EncryptUpdate.argtypes = [vp, cp, ip, cp, ctypes.c_int]
        lib.EVP_EncryptFinal_ex.argtypes = [vp, cp, ip]
        lib.OpenSSL_version.restype = cp
        return lib
    except (OSError, AttributeError):
        return None


def libcrypto_ocb(lib, key, nonce, pt, aad=b"", tag_bytes=16):
    """``(ciphertext, tag)`` of AES-OCB3 by libcrypto."""
    cipher = {16: lib.EVP_aes_128_ocb, 24: lib.EVP_aes_192_ocb, 32: lib.EVP_aes_256_ocb}[len(key)]()
    ctx = lib.EVP_CIPHER_CTX_new()
    try:
        assert lib.EVP_EncryptInit_ex(ctx, cipher, None, None, None) == 1
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_AEAD_SET_IVLEN, len(nonce), None) == 1
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_AEAD_SET_TAG, tag_bytes, None) == 1
        assert lib.EVP_EncryptInit_ex(ctx, None, None, key, nonce) == 1
        n = ctypes.c_int(0)
        if aad:
            assert lib.EVP_EncryptUpdate(ctx, None, ctypes.byref(n), aad, len(aad)) == 1
        out, got = ctypes.create_string_buffer(len(pt) + 32), 0
        if pt:
            assert lib.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), pt, len(pt)) == 1
            got = n.value
        fin = ctypes.create_string_buffer(32)
        assert lib.EVP_EncryptFinal_ex(ctx, fin, ctypes.byref(n)) == 1
        ct = out.raw[:got] + fin.raw[: n.value]
        assert len(ct) == len(pt)
        t = ctypes.create_string_buffer(16)
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_AEAD_GET_TAG, tag_bytes, t) == 1
        return ct, t.raw[:tag_bytes]
    finally:
        lib.EVP_CIPHER_CTX_free(ctx)


def cases():
    """(name, key, nonce, aad, pt, tag_bytes) of every vector."""
    for bits in (128, 192, 256):
        key = bytes(range(bits // 8))
        for i, (al, pl) in enumerate(RFC_LENGTHS):
            nonce = bytes.fromhex("BBAA9988776655443322110%X" % i)
            yield f"aes{bits}-rfc7253-a-{i:02d}", key, nonce, bytes(range(al)), bytes(range(pl)), 16
        for nl in (1, 8, 15):
            for tl in (8, 12, 16):
                nonce = bytes(0xF0 - k for k in range(nl))
                yield f"aes{bits}-nonce{nl}-tag{tl}", key, nonce, bytes(range(24)), bytes(range(40)), tl


def generate(lib):
    vectors = []
    for name, key, nonce, aad, pt, tl in cases():
        ct, tag = libcrypto_ocb(lib, key, nonce, pt, aad, tl)
        vectors.append({"name": name, "key": key.hex(), "nonce": nonce.hex(), "aad": aad.hex(), "pt": pt.hex(),
                        "tag_bytes": tl, "ct": ct.hex(), "tag": tag.hex()})
    version = lib.OpenSSL_version(0).decode().split(" ")[1]
    return {"source": "RFC 7253 Appendix A (inputs: the keys 00 01 02 .. of 16, 24 and 32 bytes, the nonces "
                      "BBAA99887766554433221100 + case, A and P the bytes 00 01 02 .. in the appendix's sixteen "
                      "combinations of 0 to 40 bytes) and nonces of 1, 8 and 15 bytes with tags of 8, 12 and 16; every "
                      f"output produced by libcrypto (OpenSSL {version}): EVP_aes_128_ocb, EVP_aes_192_ocb, "
                      "EVP_aes_256_ocb with EVP_CTRL_AEAD_SET_IVLEN and EVP_CTRL_AEAD_SET_TAG (tools/gen_ocb_vectors.py)",
            "ocb": vectors}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--check", action="store_true", help="compare the golden file with a fresh run instead of writing it")
    args = ap.parse_args()
    lib = load_libcrypto()
    if lib is None:
        sys.exit("libcrypto with the OCB ciphers is not installed")
    doc = generate(lib)
    if args.check:
        with open(GOLDEN) as f:
            have = json.load(f)
        sys.exit(0 if have["ocb"] == doc["ocb"] else "the golden file differs from libcrypto's results")
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{GOLDEN}: {len(doc['ocb'])} vectors")


if __name__ == "__main__":
    main()
