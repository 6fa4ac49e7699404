"""The BFV calls on host arrays (zkfhe.h: encryption, evaluation, threshold keys and shares, refresh and key switching, slots and
rotations, ring packing, linear transforms) as Context's _BfvCalls, and the host-only bfv_* functions."""
import ctypes
import os

import numpy as np

from .core import call


class _BfvCalls:
    # ------------------------------------------------------------------ BFV keygen / encrypt / decrypt (zkfhe.h, bfv_enc.hip)
    # Polynomials are uint64 arrays of N residues in [0, Q), CircuitInput order (highest degree first); params = (n, q, t, b).

    @staticmethod
    def _seed(seed, what, fresh=False):
        if seed is None and not fresh:
            raise ValueError("the %s is required" % what)
        seed = os.urandom(32) if seed is None else bytes(seed)
        if len(seed) != 32:
            raise ValueError("the %s is 32 bytes" % what)
        return seed

    def _sk(self, params, sk):
        sk = np.ascontiguousarray(sk, dtype=np.uint64)
        if sk.size != int(params[0]):
            raise ValueError("sk must hold N coefficients")
        return sk

    def _relin_rows(self, params, base_bits):
        return bfv_relin_digits(params, base_bits) if 1 <= int(base_bits) <= 32 else 0   # else the call refuses base_bits itself

    def bfv_fhe_keypair(self, params, seed=None):
        """zkfhe_bfv_fhe_keypair -> (sk, pk0, pk1).  seed: 32 secret bytes (None: os.urandom)."""
        n = int(params[0])
        seed = self._seed(seed, "key-generation seed", fresh=True)
        out = [np.empty(n, dtype=np.uint64) for _ in range(3)]
        self._call("zkfhe_bfv_fhe_keypair", params, seed, *out)
        return tuple(out)

    def bfv_encrypt(self, params, pk0, pk1, m, seed=None, first_index=0):
        """zkfhe_bfv_encrypt: m of shape (N,) or (n_msgs, N) -> dict u, e0, e1, c0, c1 of shape (n_msgs, N).  seed: 32 SECRET, FRESH
        bytes (None: os.urandom); reusing a (seed, index) pair reuses u (zkfhe.h)."""
        n = int(params[0])
        pk0 = np.ascontiguousarray(pk0, dtype=np.uint64)
        pk1 = np.ascontiguousarray(pk1, dtype=np.uint64)
        m = np.ascontiguousarray(m, dtype=np.uint64).reshape(-1, n)
        if pk0.size != n or pk1.size != n:
            raise ValueError("pk0 / pk1 must hold N coefficients")
        seed = self._seed(seed, "encryption seed", fresh=True)
        names = ("u", "e0", "e1", "c0", "c1")
        out = {k: np.empty(m.shape, dtype=np.uint64) for k in names}
        self._call("zkfhe_bfv_encrypt", params, pk0, pk1, m.shape[0], m, seed, int(first_index), *[out[k] for k in names])
        return out

    def bfv_decrypt(self, params, sk, c0, c1):
        """zkfhe_bfv_decrypt: c0, c1 of shape (N,) or (n_msgs, N) -> m as residues mod Q, shape (n_msgs, N)."""
        n = int(params[0])
        sk = np.ascontiguousarray(sk, dtype=np.uint64)
        c0 = np.ascontiguousarray(c0, dtype=np.uint64).reshape(-1, n)
        c1 = np.ascontiguousarray(c1, dtype=np.uint64).reshape(-1, n)
        if sk.size != n or c0.shape != c1.shape:
            raise ValueError("sk must hold N coefficients and c0, c1 the same shape")
        out = np.empty(c0.shape, dtype=np.uint64)
        self._call("zkfhe_bfv_decrypt", params, sk, c0.shape[0], c0, c1, out)
        return out

    # ------------------------------------------------------------------ BFV evaluation (zkfhe.h, bfv_eval.hip)
    # Ciphertext components are (n, N) or (N,) uint64 arrays of residues; results are (n, N) like the encrypt wrappers' (bfv_sum: (N,)).

    def _eval_arrays(self, params, *arrs):
        n = int(params[0])
        out = [np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, n) for a in arrs]
        if any(a.shape != out[0].shape for a in out):
            raise ValueError("ciphertext components must have the same shape (n, N)")
        return out

    def _plain(self, params, m, n_cts):
        n = int(params[0])
        m = np.ascontiguousarray(m, dtype=np.uint64)
        m2 = m.reshape(-1, n)
        if m.ndim == 2 and m2.shape[0] not in (1, n_cts):
            raise ValueError("m must be one plaintext (N,) or one per ciphertext (n, N)")
        return m2

    def bfv_add(self, params, a0, a1, b0, b1, subtract=False):
        """zkfhe_bfv_add: (a0 + b0, a1 + b1) mod Q, or a - b with subtract=True; every input (n, N)."""
        a0, a1, b0, b1 = self._eval_arrays(params, a0, a1, b0, b1)
        out = [np.empty(a0.shape, dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_add", params, a0.shape[0], a0, a1, b0, b1, int(bool(subtract)), *out)
        return tuple(out)

    def bfv_sum(self, params, c0, c1):
        """zkfhe_bfv_sum: the sum of all n ciphertexts (c0, c1 of shape (n, N)) as one ciphertext (two arrays of N)."""
        c0, c1 = self._eval_arrays(params, c0, c1)
        out = [np.empty(c0.shape[1], dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_sum", params, c0.shape[0], c0, c1, *out)
        return tuple(out)

    def _plain_op(self, fn, params, c0, c1, m):
        c0, c1 = self._eval_arrays(params, c0, c1)
        m = self._plain(params, m, c0.shape[0])
        out = [np.empty(c0.shape, dtype=np.uint64) for _ in range(2)]
        self._call(fn, params, c0.shape[0], c0, c1, m.shape[0], m, *out)
        return tuple(out)

    def bfv_add_plain(self, params, c0, c1, m):
        """zkfhe_bfv_add_plain: (c0 + floor(Q/T) m, c1); m is one plaintext (N,) for every ciphertext or one per ciphertext (n, N)."""
        return self._plain_op("zkfhe_bfv_add_plain", params, c0, c1, m)

    def bfv_mul_plain(self, params, c0, c1, m):
        """zkfhe_bfv_mul_plain: (c0 m, c1 m) mod (x^N + 1, Q); m as for bfv_add_plain."""
        return self._plain_op("zkfhe_bfv_mul_plain", params, c0, c1, m)

    def bfv_relin_keygen(self, params, sk, seed=None, base_bits=16):
        """zkfhe_bfv_relin_keygen -> (rlk0, rlk1) of shape (l, N), l = bfv_relin_digits(params, base_bits).  seed: 32 SECRET bytes
        (None: os.urandom); the key itself is public."""
        n, sk = int(params[0]), self._sk(params, sk)
        seed = self._seed(seed, "relinearization-key seed", fresh=True)
        out = [np.empty((self._relin_rows(params, base_bits), n), dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_relin_keygen", params, sk, seed, int(base_bits), *out)
        return tuple(out)

    def bfv_mul(self, params, a0, a1, b0, b1, rlk0, rlk1, base_bits=16):
        """zkfhe_bfv_mul: n relinearized products a * b (every input (n, N)) under the key (rlk0, rlk1) made with base_bits."""
        a0, a1, b0, b1 = self._eval_arrays(params, a0, a1, b0, b1)
        n = int(params[0])
        rlk0 = np.ascontiguousarray(rlk0, dtype=np.uint64)
        rlk1 = np.ascontiguousarray(rlk1, dtype=np.uint64)
        l = self._relin_rows(params, base_bits) or rlk0.shape[0]   # else the call refuses base_bits
        if rlk0.shape != (l, n) or rlk1.shape != (l, n):
            raise ValueError("rlk0 and rlk1 must have shape (l, N) = (%d, %d) for base_bits %d" % (l, n, base_bits))
        out = [np.empty(a0.shape, dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_mul", params, a0.shape[0], a0, a1, b0, b1, rlk0, rlk1, int(base_bits), *out)
        return tuple(out)

    def _dot_arrays(self, params, x, y, what):
        """two arrays of one operand of an inner product, (n_terms, N) or (n_groups, n_terms, N) -> ((groups, n_terms, N) views, ndim)"""
        n = int(params[0])
        x = np.ascontiguousarray(x, dtype=np.uint64)
        y = np.ascontiguousarray(y, dtype=np.uint64)
        if x.shape != y.shape or x.ndim not in (2, 3) or x.shape[-1] != n or 0 in x.shape:
            raise ValueError("%s must have the same shape (n_terms, N) or (n_groups, n_terms, N)" % what)
        return x.reshape(-1, x.shape[-2], n), y.reshape(-1, x.shape[-2], n), x.ndim

    def _dot_operands(self, params, a, b, names):
        a0, a1, a_dim = self._dot_arrays(params, a[0], a[1], names[0])
        b0, b1, b_dim = self._dot_arrays(params, b[0], b[1], names[1])
        if b0.shape[1] != a0.shape[1] or b_dim > a_dim:
            raise ValueError("%s must hold the n_terms = %d of %s, as (n_terms, N)%s" %
                             (names[1], a0.shape[1], names[0], " (shared by every group) or (n_groups, n_terms, N)" if a_dim == 3 else ""))
        out = [np.empty((a0.shape[0], a0.shape[2]) if a_dim == 3 else a0.shape[2], dtype=np.uint64) for _ in range(2)]
        return a0, a1, b0, b1, out

    def bfv_dot(self, params, a0, a1, b0, b1, rlk0, rlk1, base_bits=16):
        """zkfhe_bfv_dot: the inner product sum_i a_i * b_i of relinearized products, rescaled and relinearized once per sum, under
        the key (rlk0, rlk1) made with base_bits.  a0, a1 of shape (n_terms, N) give one ciphertext (two arrays of N); of shape
        (n_groups, n_terms, N) one per group, (n_groups, N).  b0, b1: like a, or (n_terms, N) beside a 3-D a: one b vector shared
        by every group.  n_terms is at most bfv_dot_max_terms(params)."""
        a0, a1, b0, b1, out = self._dot_operands(params, (a0, a1), (b0, b1), ("a0 and a1", "b0 and b1"))
        n = int(params[0])
        rlk0 = np.ascontiguousarray(rlk0, dtype=np.uint64)
        rlk1 = np.ascontiguousarray(rlk1, dtype=np.uint64)
        l = self._relin_rows(params, base_bits) or rlk0.shape[0]   # else the call refuses base_bits
        if rlk0.shape != (l, n) or rlk1.shape != (l, n):
            raise ValueError("rlk0 and rlk1 must have shape (l, N) = (%d, %d) for base_bits %d" % (l, n, base_bits))
        self._call("zkfhe_bfv_dot", params, a0.shape[0], a0.shape[1], a0, a1, b0.shape[0], b0, b1, rlk0, rlk1, int(base_bits), *out)
        return tuple(out)

    def bfv_dot_plain(self, params, c0, c1, m):
        """zkfhe_bfv_dot_plain: the weighted sum sum_i c_i * m_i mod (x^N + 1, Q) with public plaintexts m_i, bit for bit the bfv_sum
        of the bfv_mul_plain products.  Shapes as for bfv_dot: c0, c1 (n_terms, N) or (n_groups, n_terms, N); m like c, or
        (n_terms, N) beside a 3-D c: one weight vector shared by every group.  n_terms is at most bfv_dot_max_terms(params, True)."""
        c0, c1, m, _, out = self._dot_operands(params, (c0, c1), (m, m), ("c0 and c1", "m"))
        self._call("zkfhe_bfv_dot_plain", params, c0.shape[0], c0.shape[1], c0, c1, m.shape[0], m, *out)
        return tuple(out)

    def bfv_noise(self, params, sk, c0, c1):
        """zkfhe_bfv_noise: per ciphertext, max |[c0 + c1 s - floor(Q/T) m]_Q| with m the decryption; shape (n,)."""
        sk = self._sk(params, sk)
        c0, c1 = self._eval_arrays(params, c0, c1)
        out = np.empty(c0.shape[0], dtype=np.uint64)
        self._call("zkfhe_bfv_noise", params, sk, c0.shape[0], c0, c1, out)
        return out

    # ------------------------------------------------------------------ threshold BFV (zkfhe.h, bfv_threshold.hip)
    # Party i holds sk_i; keys and shares are uint64 arrays of residues like the calls above.  Every seed is 32 SECRET bytes
    # (the CRS seed is public); a None share seed draws os.urandom(32).

    def bfv_keygen_share(self, params, crs_seed, party_seed):
        """zkfhe_bfv_keygen_share -> (sk_i, pk0_share, pk1): pk0_share = -(a s_i + e_i), pk1 = a from the public crs_seed."""
        n = int(params[0])
        crs_seed, party_seed = self._seed(crs_seed, "CRS seed"), self._seed(party_seed, "party seed")
        out = [np.empty(n, dtype=np.uint64) for _ in range(3)]
        self._call("zkfhe_bfv_keygen_share", params, crs_seed, party_seed, *out)
        return tuple(out)

    def bfv_share_aggregate(self, params, shares):
        """zkfhe_bfv_share_aggregate: shares of shape (P, N) or (P, n_polys, N) -> their sum mod Q, shape (N,) or (n_polys, N)."""
        n = int(params[0])
        shares = np.ascontiguousarray(shares, dtype=np.uint64)
        if shares.ndim not in (2, 3) or shares.shape[-1] != n:
            raise ValueError("shares must have shape (P, N) or (P, n_polys, N)")
        s3 = shares.reshape(shares.shape[0], shares.shape[1] if shares.ndim == 3 else 1, n)   # P = 0 is refused by the call
        out = np.empty(s3.shape[1:], dtype=np.uint64)
        self._call("zkfhe_bfv_share_aggregate", params, s3.shape[0], s3.shape[1], s3, out)
        return out.reshape(shares.shape[1:])

    def bfv_relin_share1(self, params, sk, crs_seed, party_seed, base_bits=8):
        """zkfhe_bfv_relin_share1 -> (h0_i, h1_i) of shape (l, N): round 1 of the collective relinearization key."""
        n, sk = int(params[0]), self._sk(params, sk)
        crs_seed, party_seed = self._seed(crs_seed, "CRS seed"), self._seed(party_seed, "party seed")
        out = [np.empty((self._relin_rows(params, base_bits), n), dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_relin_share1", params, sk, crs_seed, party_seed, int(base_bits), *out)
        return tuple(out)

    def bfv_relin_share2(self, params, sk, party_seed, h0, h1, base_bits=8):
        """zkfhe_bfv_relin_share2 -> r_i of shape (l, N) from the round-1 aggregates h0, h1 (l, N); rlk0 = bfv_share_aggregate of
        the r_i, rlk1 = h1.  party_seed must be the one of round 1."""
        n, sk = int(params[0]), self._sk(params, sk)
        party_seed = self._seed(party_seed, "party seed")
        h0 = np.ascontiguousarray(h0, dtype=np.uint64)
        h1 = np.ascontiguousarray(h1, dtype=np.uint64)
        l = self._relin_rows(params, base_bits)
        if l and (h0.shape != (l, n) or h1.shape != (l, n)):
            raise ValueError("h0 and h1 must have shape (l, N) = (%d, %d) for base_bits %d" % (l, n, base_bits))
        out = np.empty((l, n), dtype=np.uint64)
        self._call("zkfhe_bfv_relin_share2", params, sk, party_seed, int(base_bits), h0, h1, out)
        return out

    def bfv_decrypt_share(self, params, sk, c1, seed=None, first_index=0, smudge_bound=0):
        """zkfhe_bfv_decrypt_share: c1 of shape (N,) or (n, N) -> d_j = c1_j s_i + e_j, shape (n, N); e_j uniform in
        [-smudge_bound, smudge_bound] from (seed, 9, first_index + j).  seed: 32 SECRET bytes (None: os.urandom); never reuse a
        (seed, index) pair on a different c1."""
        n, sk = int(params[0]), self._sk(params, sk)
        seed = self._seed(seed, "share seed", fresh=True)
        c1 = np.ascontiguousarray(c1, dtype=np.uint64).reshape(-1, n)
        out = np.empty(c1.shape, dtype=np.uint64)
        self._call("zkfhe_bfv_decrypt_share", params, sk, c1.shape[0], c1, seed, int(first_index), int(smudge_bound), out)
        return out

    def bfv_decrypt_combine(self, params, c0, shares):
        """zkfhe_bfv_decrypt_combine: c0 of shape (N,) or (n, N) and the parties' shares (P, n, N) (or (P, N)) -> m as residues mod Q,
        shape (n, N): the rounding of bfv_decrypt applied to [c0 + sum_i d_i]_Q."""
        n = int(params[0])
        c0 = np.ascontiguousarray(c0, dtype=np.uint64).reshape(-1, n)
        d = np.ascontiguousarray(shares, dtype=np.uint64)
        d = d.reshape(d.shape[0], 1, n) if d.ndim == 2 else d
        if d.ndim != 3 or d.shape[1:] != c0.shape:
            raise ValueError("shares must have shape (P, n, N) for c0 of shape (n, N)")
        out = np.empty(c0.shape, dtype=np.uint64)
        self._call("zkfhe_bfv_decrypt_combine", params, d.shape[0], c0.shape[0], c0, d, out)
        return out

    # ------------------------------------------------------------------ collective refresh and key switching (zkfhe.h, bfv_refresh.hip)
    # Shapes follow bfv_decrypt_share / bfv_decrypt_combine: c0, c1 of shape (N,) or (n, N), shares (P, n, N) (or (P, N)).  Share
    # seeds are 32 SECRET bytes (None: os.urandom); never reuse a (seed, index) pair.  A refresh's crs_seed and first_index are
    # public, the same for every party and the combiner, and differ between refreshes.

    def _share_planes(self, c0, h0, h1):
        out = []
        for h in (h0, h1):
            h = np.ascontiguousarray(h, dtype=np.uint64)
            h = h.reshape(h.shape[0], 1, c0.shape[1]) if h.ndim == 2 else h
            if h.ndim != 3 or h.shape[1:] != c0.shape:
                raise ValueError("shares must have shape (P, n, N) for c0 of shape (n, N)")
            out.append(h)
        if out[0].shape != out[1].shape:
            raise ValueError("h0 and h1 shares must come from the same parties")
        return out

    def bfv_pcks_share(self, params, sk, pk0_to, pk1_to, c1, seed=None, first_index=0, smudge_bound=0):
        """zkfhe_bfv_pcks_share: c1 of shape (N,) or (n, N) -> (h0, h1) of shape (n, N): h0_j = s_i c1_j + u_j pk0_to + e0_j,
        h1_j = u_j pk1_to + e1_j, towards the public key (pk0_to, pk1_to); e0_j uniform in [-smudge_bound, smudge_bound]."""
        n, sk = int(params[0]), self._sk(params, sk)
        pk0_to = np.ascontiguousarray(pk0_to, dtype=np.uint64)
        pk1_to = np.ascontiguousarray(pk1_to, dtype=np.uint64)
        if pk0_to.size != n or pk1_to.size != n:
            raise ValueError("pk0_to / pk1_to must hold N coefficients")
        seed = self._seed(seed, "share seed", fresh=True)
        c1 = np.ascontiguousarray(c1, dtype=np.uint64).reshape(-1, n)
        out = [np.empty(c1.shape, dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_pcks_share", params, sk, pk0_to, pk1_to, c1.shape[0], c1, seed, int(first_index), int(smudge_bound), *out)
        return tuple(out)

    def bfv_pcks_combine(self, params, c0, h0_shares, h1_shares):
        """zkfhe_bfv_pcks_combine: c0 of shape (N,) or (n, N) and the parties' shares (P, n, N) (or (P, N)) -> (c0', c1') of shape
        (n, N), the same plaintext under the key the shares were made towards: c0' = c0 + sum_i h0_i, c1' = sum_i h1_i."""
        c0 = np.ascontiguousarray(c0, dtype=np.uint64).reshape(-1, int(params[0]))
        h0, h1 = self._share_planes(c0, h0_shares, h1_shares)
        out = [np.empty(c0.shape, dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_pcks_combine", params, h0.shape[0], c0.shape[0], c0, h0, h1, *out)
        return tuple(out)

    def bfv_refresh_share(self, params, sk, crs_seed, c1, seed=None, first_index=0, smudge_bound=0):
        """zkfhe_bfv_refresh_share: c1 of shape (N,) or (n, N) -> (h0, h1) of shape (n, N): h0_j = s_i c1_j - delta M_j + e0_j,
        h1_j = -s_i a_j + delta M_j + e1_j, a_j from the public (crs_seed, first_index + j)."""
        n, sk = int(params[0]), self._sk(params, sk)
        crs_seed, seed = self._seed(crs_seed, "CRS seed"), self._seed(seed, "share seed", fresh=True)
        c1 = np.ascontiguousarray(c1, dtype=np.uint64).reshape(-1, n)
        out = [np.empty(c1.shape, dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_refresh_share", params, sk, crs_seed, c1.shape[0], c1, seed, int(first_index), int(smudge_bound), *out)
        return tuple(out)

    def bfv_refresh_combine(self, params, crs_seed, c0, h0_shares, h1_shares, first_index=0):
        """zkfhe_bfv_refresh_combine: c0 of shape (N,) or (n, N) and the parties' shares (P, n, N) (or (P, N)) -> the refreshed
        (c0', c1') of shape (n, N) under the same collective key; crs_seed and first_index are those of the shares."""
        c0 = np.ascontiguousarray(c0, dtype=np.uint64).reshape(-1, int(params[0]))
        crs_seed = self._seed(crs_seed, "CRS seed")
        h0, h1 = self._share_planes(c0, h0_shares, h1_shares)
        out = [np.empty(c0.shape, dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_refresh_combine", params, h0.shape[0], c0.shape[0], crs_seed, int(first_index), c0, h0, h1, *out)
        return tuple(out)

    # ------------------------------------------------------------------ slots and rotations (zkfhe.h, bfv_galois.hip)
    # Slot values and plaintexts are (n, N) uint64 arrays like the calls above; a Galois key is (gk0, gk1) of shape (l, N), and
    # bfv_slot_sum takes the keys of bfv_slot_sum_elements stacked as (log2(N), l, N).

    def _slots(self, fn, params, x):
        x = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, int(params[0]))
        out = np.empty(x.shape, dtype=np.uint64)
        self._call(fn, params, x.shape[0], x, out)
        return out

    def bfv_encode_slots(self, params, values):
        """zkfhe_bfv_encode_slots: slot values in [0, T) of shape (N,) or (n, N) -> plaintexts (n, N), centred residues mod Q."""
        return self._slots("zkfhe_bfv_encode_slots", params, values)

    def bfv_decode_slots(self, params, m):
        """zkfhe_bfv_decode_slots: plaintexts of shape (N,) or (n, N) -> slot values in [0, T), shape (n, N)."""
        return self._slots("zkfhe_bfv_decode_slots", params, m)

    def _galois_key(self, fn, params, sk, seeds, g, base_bits):
        n, sk = int(params[0]), self._sk(params, sk)
        out = [np.empty((self._relin_rows(params, base_bits), n), dtype=np.uint64) for _ in range(2)]
        self._call(fn, params, sk, *seeds, int(g), int(base_bits), *out)
        return tuple(out)

    def bfv_galois_keygen(self, params, sk, g, seed=None, base_bits=16):
        """zkfhe_bfv_galois_keygen -> (gk0, gk1) of shape (l, N): the Galois key of sk for the element g.  seed: 32 SECRET bytes
        (None: os.urandom); the key itself is public."""
        seed = self._seed(seed, "Galois-key seed", fresh=True)
        return self._galois_key("zkfhe_bfv_galois_keygen", params, sk, [seed], g, base_bits)

    def bfv_galois_share(self, params, sk, crs_seed, party_seed, g, base_bits=8):
        """zkfhe_bfv_galois_share -> (r_i, a) of shape (l, N): party i's share of the collective Galois key for g; gk0 =
        bfv_share_aggregate of the r_i, gk1 = a."""
        crs_seed, party_seed = self._seed(crs_seed, "CRS seed"), self._seed(party_seed, "party seed")
        return self._galois_key("zkfhe_bfv_galois_share", params, sk, [crs_seed, party_seed], g, base_bits)

    # ------------------------------------------------------------------ hybrid keys modulo Q P (zkfhe.h, bfv_hybrid.hip)

    def _hybrid_key(self, fn, params, p, sk, tail, base_bits):
        n, sk = int(params[0]), self._sk(params, sk)
        out = [np.empty((self._relin_rows(params, base_bits), n), dtype=np.uint64) for _ in range(4)]
        self._call(fn, params, int(p), sk, *tail, int(base_bits), *out)
        return tuple(out)

    def bfv_relin_keygen_hybrid(self, params, p, sk, seed=None, base_bits=16):
        """zkfhe_bfv_relin_keygen_hybrid -> (rlk0_q, rlk1_q, rlk0_p, rlk1_p) of shape (l, N): the relinearization key modulo Q P
        for the special modulus p as its q-planes and p-planes.  seed: 32 SECRET bytes (None: os.urandom)."""
        seed = self._seed(seed, "relinearization-key seed", fresh=True)
        return self._hybrid_key("zkfhe_bfv_relin_keygen_hybrid", params, p, sk, [seed], base_bits)

    def bfv_galois_keygen_hybrid(self, params, p, sk, g, seed=None, base_bits=16):
        """zkfhe_bfv_galois_keygen_hybrid -> (gk0_q, gk1_q, gk0_p, gk1_p) of shape (l, N): the Galois key of sk for g modulo Q P."""
        seed = self._seed(seed, "Galois-key seed", fresh=True)
        return self._hybrid_key("zkfhe_bfv_galois_keygen_hybrid", params, p, sk, [seed, int(g)], base_bits)

    def bfv_galois_share_hybrid(self, params, p, sk, crs_seed, party_seed, g, base_bits=8):
        """zkfhe_bfv_galois_share_hybrid -> (r_q, a_q, r_p, a_p) of shape (l, N): party i's share of the collective hybrid Galois key
        for g; gk0_q = bfv_share_aggregate of the r_q, gk0_p = bfv_share_aggregate of the r_p under parameters whose q is p."""
        crs_seed, party_seed = self._seed(crs_seed, "CRS seed"), self._seed(party_seed, "party seed")
        return self._hybrid_key("zkfhe_bfv_galois_share_hybrid", params, p, sk, [crs_seed, party_seed, int(g)], base_bits)

    def _galois_keys(self, params, gk0, gk1, base_bits, lead):
        n = int(params[0])
        gk0 = np.ascontiguousarray(gk0, dtype=np.uint64)
        gk1 = np.ascontiguousarray(gk1, dtype=np.uint64)
        l = self._relin_rows(params, base_bits) or (gk0.shape[-2] if gk0.ndim >= 2 else 0)   # else the call refuses base_bits
        if gk0.shape != lead + (l, n) or gk1.shape != lead + (l, n):
            raise ValueError("gk0 and gk1 must have shape %s for base_bits %d" % (lead + (l, n), base_bits))
        return gk0, gk1

    def bfv_apply_galois(self, params, c0, c1, g, gk0, gk1, base_bits=16):
        """zkfhe_bfv_apply_galois: n ciphertexts (n, N) -> sigma_g of each, key-switched back to s with (gk0, gk1) of shape (l, N)."""
        c0, c1 = self._eval_arrays(params, c0, c1)
        gk0, gk1 = self._galois_keys(params, gk0, gk1, base_bits, ())
        out = [np.empty(c0.shape, dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_apply_galois", params, c0.shape[0], c0, c1, int(g), gk0, gk1, int(base_bits), *out)
        return tuple(out)

    def bfv_slot_sum(self, params, c0, c1, gk0, gk1, base_bits=16):
        """zkfhe_bfv_slot_sum: n ciphertexts (n, N) -> every slot holds the total, with the keys of bfv_slot_sum_elements stacked
        as gk0, gk1 of shape (log2(N), l, N)."""
        c0, c1 = self._eval_arrays(params, c0, c1)
        gk0, gk1 = self._galois_keys(params, gk0, gk1, base_bits, (int(params[0]).bit_length() - 1,))
        out = [np.empty(c0.shape, dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_slot_sum", params, c0.shape[0], c0, c1, gk0, gk1, int(base_bits), *out)
        return tuple(out)

    # ------------------------------------------------------------------ ring packing (zkfhe.h, bfv_pack.hip)

    @staticmethod
    def _exponents(k, what):
        k = np.ascontiguousarray(k, dtype=np.uint64)
        if k.ndim > 1:
            raise ValueError("%s must be one integer or one per ciphertext" % what)
        return k.reshape(-1)

    def bfv_mul_monomial(self, params, c0, c1, k):
        """zkfhe_bfv_mul_monomial: n ciphertexts (n, N) -> x^k times each, mod (x^N + 1, Q); k is one exponent below 2N for every
        ciphertext or one per ciphertext."""
        c0, c1 = self._eval_arrays(params, c0, c1)
        k = self._exponents(k, "k")
        out = [np.empty(c0.shape, dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_mul_monomial", params, c0.shape[0], c0, c1, k.shape[0], k, *out)
        return tuple(out)

    def bfv_pack(self, params, c0, c1, gk0, gk1, pos=None, base_bits=16):
        """zkfhe_bfv_pack: c0, c1 of shape (n, N) (one group) or (n_groups, n, N) -> (out0, out1) of shape (n_groups, N): coefficient
        i N / n' of result g is coefficient pos[g][i] (None: 0) of input i of group g, every other coefficient 0.  gk0, gk1: the keys
        of bfv_pack_elements stacked as (log2(N), l, N)."""
        n = int(params[0])
        c0 = np.ascontiguousarray(c0, dtype=np.uint64)
        c1 = np.ascontiguousarray(c1, dtype=np.uint64)
        if c0.shape != c1.shape or c0.ndim not in (2, 3) or c0.shape[-1] != n or 0 in c0.shape:
            raise ValueError("c0 and c1 must have the same shape (n, N) or (n_groups, n, N)")
        n_groups, n_in = (1, c0.shape[0]) if c0.ndim == 2 else c0.shape[:2]
        p = None
        if pos is not None:
            p = np.ascontiguousarray(pos, dtype=np.uint64)
            if p.size != n_groups * n_in:
                raise ValueError("pos must hold one position per input")
        gk0, gk1 = self._galois_keys(params, gk0, gk1, base_bits, (n.bit_length() - 1,))
        out = [np.empty((n_groups, n), dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_pack", params, n_groups, n_in, c0, c1, p, gk0, gk1, int(base_bits), *out)
        return tuple(out)

    # ------------------------------------------------------------------ encrypted matrix-vector products (zkfhe.h, bfv_linear.hip)
    # elements: K Galois elements (repeats allowed); their keys stacked as gk0, gk1 of shape (K, l, N) (the rows of g = 1 are not read).

    def _elements(self, params, elements, gk0, gk1, base_bits):
        g = np.ascontiguousarray([int(x) for x in elements], dtype=np.uint64).reshape(-1)
        gk0, gk1 = self._galois_keys(params, gk0, gk1, base_bits, (g.shape[0],))
        return g, gk0, gk1

    def bfv_apply_galois_many(self, params, c0, c1, elements, gk0, gk1, base_bits=16):
        """zkfhe_bfv_apply_galois_many: n ciphertexts (n, N) -> (out0, out1) of shape (K, n, N), block k the hoisted rotation of
        every ciphertext by elements[k] (the digits of c1 are decomposed and transformed once)."""
        c0, c1 = self._eval_arrays(params, c0, c1)
        g, gk0, gk1 = self._elements(params, elements, gk0, gk1, base_bits)
        out = [np.empty((g.shape[0],) + c0.shape, dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_apply_galois_many", params, c0.shape[0], c0, c1, g.shape[0], g, gk0, gk1, int(base_bits), *out)
        return tuple(out)

    def bfv_linear_transform(self, params, c0, c1, elements, gk0, gk1, diagonals, base_bits=16):
        """zkfhe_bfv_linear_transform: n ciphertexts (n, N) -> sum_k diagonals[k] * (the hoisted rotation by elements[k]), shape
        (n, N).  diagonals: K plaintexts (K, N), shared by every ciphertext (bfv_encode_slots of the slot-value diagonals)."""
        c0, c1 = self._eval_arrays(params, c0, c1)
        g, gk0, gk1 = self._elements(params, elements, gk0, gk1, base_bits)
        d = np.ascontiguousarray(diagonals, dtype=np.uint64)
        if d.shape != (g.shape[0], int(params[0])):
            raise ValueError("diagonals must have shape (K, N), one plaintext per element")
        out = [np.empty(c0.shape, dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_linear_transform", params, c0.shape[0], c0, c1, g.shape[0], g, gk0, gk1, int(base_bits), d, *out)
        return tuple(out)

    def bfv_linear_transform_bsgs(self, params, c0, c1, baby_elements, bk0, bk1, giant_elements, hk0, hk1, diagonals, base_bits=16):
        """zkfhe_bfv_linear_transform_bsgs: n ciphertexts (n, N) -> sum_i (the hoisted rotation by giant_elements[i] of sum_j
        diagonals[i][j] * (the hoisted rotation by baby_elements[j])), shape (n, N).  bk0, bk1: the baby keys (n_baby, l, N); hk0, hk1:
        the giant keys (n_giant, l, N); diagonals: plaintexts (n_giant, n_baby, N), already rotated by the inverse of their giant
        step and shared by every ciphertext (bfv_encode_slots of the slot values of bfv_matrix_bsgs)."""
        c0, c1 = self._eval_arrays(params, c0, c1)
        gb, bk0, bk1 = self._elements(params, baby_elements, bk0, bk1, base_bits)
        gg, hk0, hk1 = self._elements(params, giant_elements, hk0, hk1, base_bits)
        d = np.ascontiguousarray(diagonals, dtype=np.uint64)
        if d.shape != (gg.shape[0], gb.shape[0], int(params[0])):
            raise ValueError("diagonals must have shape (n_giant, n_baby, N), one plaintext per pair of elements")
        out = [np.empty(c0.shape, dtype=np.uint64) for _ in range(2)]
        self._call("zkfhe_bfv_linear_transform_bsgs", params, c0.shape[0], c0, c1, gb.shape[0], gb, bk0, bk1, gg.shape[0], gg, hk0, hk1,
                   int(base_bits), d, *out)
        return tuple(out)


# ------------------------------------------------------------------ the host-only functions: no context, no GPU

def _count_then_fill(fn, params):
    """the count-then-fill host functions: fn(&params, NULL, &count), then fn(&params, out, &count) into a uint64 array"""
    cnt = ctypes.c_size_t()
    call(fn, params, None, ctypes.byref(cnt))
    out = np.empty(cnt.value, dtype=np.uint64)
    call(fn, params, out, ctypes.byref(cnt))
    return out


def bfv_relin_digits(params, base_bits):
    """zkfhe_bfv_relin_digits (host only): l = ceil(bitlen(Q - 1) / base_bits), the rows of a relinearization key."""
    l = ctypes.c_size_t()
    call("zkfhe_bfv_relin_digits", params, int(base_bits), ctypes.byref(l))
    return l.value


def bfv_plan_bytes(params, base_bits, n_elems_total, n_key_slots, n_diagonals):
    """zkfhe_bfv_plan_bytes (host only): the device bytes of a plan, 4 (2 n_elems_total + 2 n_key_slots l N 5 + n_diagonals N 5) with
    l = bfv_relin_digits.  n_elems_total: K, or n_baby + n_giant; n_key_slots: the elements with g != 1; n_diagonals: K, or
    n_baby n_giant."""
    out = ctypes.c_uint64()
    call("zkfhe_bfv_plan_bytes", params, int(base_bits), int(n_elems_total), int(n_key_slots), int(n_diagonals), ctypes.byref(out))
    return out.value


def bfv_evk_bytes(params, base_bits, has_relin, n_galois):
    """zkfhe_bfv_evk_bytes (host only): the device bytes of a key set, (has_relin + n_galois) 2 l 5 N 4 with l = bfv_relin_digits."""
    out = ctypes.c_uint64()
    call("zkfhe_bfv_evk_bytes", params, int(base_bits), int(bool(has_relin)), int(n_galois), ctypes.byref(out))
    return out.value


def bfv_hybrid_max_p(params, base_bits):
    """zkfhe_bfv_hybrid_max_p (host only): the largest special modulus P below 2^63 with l N (2^w - 1) (Q P - 1) <= floor(P5 / 2),
    P5 the product of the five RNS primes; the gcd with Q is not looked at."""
    out = ctypes.c_uint64()
    call("zkfhe_bfv_hybrid_max_p", params, int(base_bits), ctypes.byref(out))
    return out.value


def bfv_dot_max_terms(params, plain=False):
    """zkfhe_bfv_dot_max_terms (host only): the largest n_terms of Context.bfv_dot (plain=True: of Context.bfv_dot_plain), for which
    the exact sum stays within half of the five RNS primes' product; saturates at 2^64 - 1."""
    out = ctypes.c_size_t()
    call("zkfhe_bfv_dot_max_terms", params, int(bool(plain)), ctypes.byref(out))
    return out.value


def bfv_slot_count(params):
    """zkfhe_bfv_slot_count (host only): N when T is a batching modulus (prime, below 2^31, 2N | T - 1); raises otherwise."""
    slots = ctypes.c_size_t()
    call("zkfhe_bfv_slot_count", params, ctypes.byref(slots))
    return slots.value


def bfv_galois_element(params, steps=0, swap_rows=False):
    """zkfhe_bfv_galois_element (host only): g = 5^(steps mod N/2) mod 2N (a rotation of both rows left by steps), times 2N - 1 if
    swap_rows."""
    g = ctypes.c_uint64()
    call("zkfhe_bfv_galois_element", params, int(steps), int(bool(swap_rows)), ctypes.byref(g))
    return g.value


def bfv_slot_sum_elements(params):
    """zkfhe_bfv_slot_sum_elements (host only): the log2(N) Galois elements of bfv_slot_sum in order, a list of ints."""
    return [int(x) for x in _count_then_fill("zkfhe_bfv_slot_sum_elements", params)]


def bfv_pack_elements(params):
    """zkfhe_bfv_pack_elements (host only): the log2(N) Galois elements 2^l + 1 of bfv_pack in order, a list of ints; any T."""
    return [int(x) for x in _count_then_fill("zkfhe_bfv_pack_elements", params)]


def bfv_error_cdt(params):
    """zkfhe_bfv_error_cdt (host only): the 2 B thresholds of the error sampler as a uint64 array."""
    return _count_then_fill("zkfhe_bfv_error_cdt", params)


def bfv_matrix_diagonals(params, matrix):
    """Host only, Python only: a dense N x N matrix over Z_T acting on the slot vector in slot order (slot p = row N/2 + j) ->
    (elements, diagonals) with (matrix @ v)[p] = sum_i diagonals[i][p] rot_i(v)[p] mod T, rot_i the slot permutation of
    elements[i] = 5^k (2N - 1)^swap: both rows left by k, then the rows swapped.  diagonals: slot values of shape (K, N), to be
    encoded with Context.bfv_encode_slots; all-zero diagonals are dropped (a zero matrix gives K = 0)."""
    n, t = int(params[0]), int(params[2])
    bfv_slot_count(params)   # refuses a T that does not batch
    m = np.asarray(matrix)
    if m.shape != (n, n):
        raise ValueError("matrix must have shape (N, N)")
    m = (m.astype(object) % t).astype(np.uint64) if m.dtype == object else np.mod(m, t).astype(np.uint64)
    half, p = n // 2, np.arange(n)
    row, j = p // half, p % half
    elements, diagonals = [], []
    for swap in (0, 1):
        for k in range(half):   # slot (row, j) of the rotated vector holds v[(row ^ swap, j + k)]
            d = m[p, (row ^ swap) * half + (j + k) % half]
            if d.any():
                elements.append(bfv_galois_element(params, k, bool(swap)))
                diagonals.append(d)
    return elements, np.array(diagonals, dtype=np.uint64).reshape(-1, n)


def bfv_matrix_bsgs(params, matrix, n_baby=None):
    """Host only, Python only: the baby-step/giant-step split of bfv_matrix_diagonals for Context.bfv_linear_transform_bsgs ->
    (baby_elements, giant_elements, diagonals).  Baby column b is the element 5^b, giant row (i, swap) the element 5^(i n_baby)
    (2N - 1)^swap for i < ceil((N/2) / n_baby), the swap = 0 rows first.  diagonals: slot values of shape (n_giant, n_baby, N), to be
    encoded with Context.bfv_encode_slots: entry (i, swap), b is the diagonal of k = i n_baby + b and swap (zero where k >= N/2),
    rotated by the inverse of its giant step, d'[(row, j)] = d[(row ^ swap, (j - i n_baby) mod N/2)].  n_baby defaults to
    2^ceil(log2(N) / 2); any 1 <= n_baby <= N/2 is accepted.  Giant rows that are all zero are dropped, then baby columns that are
    all zero (a zero matrix gives empty lists)."""
    n, t = int(params[0]), int(params[2])
    bfv_slot_count(params)   # refuses a T that does not batch
    m = np.asarray(matrix)
    if m.shape != (n, n):
        raise ValueError("matrix must have shape (N, N)")
    half, log_n = n // 2, n.bit_length() - 1
    n_baby = 1 << -(-log_n // 2) if n_baby is None else int(n_baby)
    if not 1 <= n_baby <= half:
        raise ValueError("n_baby must be in [1, N/2]")
    m = (m.astype(object) % t).astype(np.uint64) if m.dtype == object else np.mod(m, t).astype(np.uint64)
    p = np.arange(n)
    row, j = p // half, p % half
    steps = -(-half // n_baby)
    giants, d = [], np.zeros((2 * steps, n_baby, n), dtype=np.uint64)
    for swap in (0, 1):
        for i in range(steps):
            giants.append(bfv_galois_element(params, i * n_baby, bool(swap)))
            src = (row ^ swap) * half + (j - i * n_baby) % half   # the slot that the giant step moves to p
            for b in range(min(n_baby, half - i * n_baby)):
                k = i * n_baby + b
                d[swap * steps + i, b] = m[src, (src // half ^ swap) * half + (src % half + k) % half]
    keep_g = [i for i in range(2 * steps) if d[i].any()]
    d = d[keep_g]
    keep_b = [b for b in range(n_baby) if d[:, b].any()]
    return [bfv_galois_element(params, b, False) for b in keep_b], [giants[i] for i in keep_g], np.ascontiguousarray(d[:, keep_b])
