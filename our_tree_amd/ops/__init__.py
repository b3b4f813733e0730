"""Device ops (gfx950 HIP kernels) on torch tensors."""
from ._common import IMPLS
from .aes_ops import (CtrStream, cbc_decrypt, cbc_decrypt_segments, cbc_encrypt_segments, cfb128_decrypt,
                      cfb128_decrypt_segments, cfb128_encrypt_segments, ctr, ctr32, ctr_rfc3686, ecb_decrypt,
                      ecb_encrypt, last_impl, pick_impl, split_fallback_reason, xts_decrypt, xts_encrypt)
from .batch_ops import (CtrBatch, GcmBatch, ctr_batch, gcm_batch_spans, gcm_decrypt_batch, gcm_encrypt_batch,
                        ghash_batch)
from .chacha_ops import (ChaChaTagError, chacha20, chacha20_poly1305_decrypt, chacha20_poly1305_encrypt, poly1305,
                         poly1305_spans)
from . import chacha_batch_ops  # batched ChaCha20-Poly1305: its names are not in __all__ yet (docs/API.md)
from . import ocb_ops  # AES-OCB3: its names are not in __all__ yet either (docs/API.md)
from . import ocb_batch_ops  # batched AES-OCB3: the same arrangement (docs/API.md)
from . import ccm_batch_ops  # batched AES-CCM and its single-message calls: the same arrangement (docs/API.md)
from . import gcm_siv_ops  # AES-GCM-SIV and POLYVAL: the same arrangement (docs/API.md)
from . import gcm_siv_batch_ops  # batched AES-GCM-SIV: the same arrangement (docs/API.md)
from . import gcm_mk_batch_ops  # batched AES-GCM with a key per record: the same arrangement (docs/API.md)
from .gcm_ops import GcmTagError, gcm_decrypt, gcm_encrypt, ghash, ghash_spans
from .keys import expand_key
from .stream_ops import checksum, clock_ghz, clock_probe, fill_random_, rc4_crypt_batch, rc4_multi, rc4_states, xor

__all__ = [  # one module per paragraph, in the order of the imports
    "IMPLS",
    "pick_impl", "last_impl", "split_fallback_reason", "ctr", "ctr_rfc3686", "ctr32", "CtrStream", "ecb_encrypt",
    "ecb_decrypt", "cbc_decrypt", "cfb128_decrypt", "cbc_encrypt_segments", "cbc_decrypt_segments",
    "cfb128_encrypt_segments", "cfb128_decrypt_segments", "xts_encrypt", "xts_decrypt",
    "CtrBatch", "ctr_batch", "GcmBatch", "gcm_encrypt_batch", "gcm_decrypt_batch", "ghash_batch", "gcm_batch_spans",
    "chacha20", "poly1305", "poly1305_spans", "chacha20_poly1305_encrypt", "chacha20_poly1305_decrypt", "ChaChaTagError",
    "ghash", "ghash_spans", "gcm_encrypt", "gcm_decrypt", "GcmTagError",
    "expand_key",
    "xor", "rc4_multi", "rc4_states", "rc4_crypt_batch", "fill_random_", "checksum", "clock_probe", "clock_ghz",
]
