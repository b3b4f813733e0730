"""Cipher "model families": AES (ECB/CBC/CFB128/CTR, 128/192/256), AES-XTS, AES-GCM, ChaCha20-Poly1305 and ARC4/RC4."""
from . import cpu_ref
from .aes import AES, AESGCM, AESXTS, DIR_BOTH, DIR_DECRYPT, DIR_ENCRYPT, DIR_NONE
from .arc4 import ARC4, RC4MultiStream
from .chacha import ChaCha20Poly1305

__all__ = ["AES", "AESGCM", "AESXTS", "ChaCha20Poly1305", "ARC4", "RC4MultiStream", "cpu_ref", "DIR_NONE", "DIR_ENCRYPT", "DIR_DECRYPT", "DIR_BOTH"]
