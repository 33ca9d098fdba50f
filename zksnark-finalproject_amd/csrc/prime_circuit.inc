// PrimeCircuit (BASELINE configs[4]) — C++ mirror of the reference's Fermat-prime circuit, included into circuits.hip's
// anonymous namespace (it builds on `Circuit` / `Lc`).  Host only.
//   PrimeCircuit::generate_constraints     /root/reference/src/arkworks/prime_snark/prime_circut.rs:92-146
//   FermatCircuit + modpow                 /root/reference/src/arkworks/prime_snark/fermat_circut.rs:38-130
//   hashed Fermat bases, x+j hashing        /root/reference/src/arkworks/prime_snark/utils/hasher.rs:28-111
//   witnessed quotients / square-and-multiply  .../utils/modulo.rs:24-89, modpow_circut.rs:134-160 (struct_initializer)
//   native search                           prime_circut.rs:147-195, backend/prime_snark.rs:49-105
//   constants K = 3, NUM_BITS = 20          .../utils/constants.rs:4-9
// The gadgets the reference pulls from un-vendored crates are restated from their published semantics (ark-r1cs-std 0.4:
// Boolean / UInt8 / UInt32::addmany / FpVar::{to_bits_le, to_bytes, is_eq, inverse, is_cmp_unchecked};
// ark-crypto-primitives 0.4 crh::sha256::constraints::{Sha256Gadget, DigestVar}).  What IS checked here: digests equal
// hashlib.sha256, the modular exponentiations equal Python's pow, the system is satisfied, proofs verify
// (tests/test_prime_circuit.py).  What cannot be checked offline: that variable k / constraint k are upstream's
// variable k / constraint k — the constraint LAYOUT is a restatement, parity with upstream's layout is unpinned (DESIGN.md).

// ------------------------------------------------------------------------------------------------ native helpers
struct Sha256Native {
    uint32_t h[8];
    uint8_t buf[64];
    size_t fill = 0;
    uint64_t total = 0;
    static constexpr uint32_t K_[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
        0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
        0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
        0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
        0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
        0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    static constexpr uint32_t H0[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    Sha256Native() { for (int i = 0; i < 8; i++) h[i] = H0[i]; }
    static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
    void block(const uint8_t *p) {
        uint32_t w[64];
        for (int i = 0; i < 16; i++) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
        for (int i = 16; i < 64; i++) {
            const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; i++) {
            const uint32_t t0 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K_[i] + w[i];
            const uint32_t t1 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t0; d = c; c = b; b = a; a = t0 + t1;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    void update(const uint8_t *p, size_t n) {
        total += n;
        while (n) {
            const size_t k = std::min(n, 64 - fill);
            memcpy(buf + fill, p, k);
            fill += k; p += k; n -= k;
            if (fill == 64) { block(buf); fill = 0; }
        }
    }
    void finalize(uint8_t out[32]) {
        const uint64_t bits = total * 8;
        uint8_t pad[72] = {0x80};
        const size_t padlen = (fill < 56 ? 56 : 120) - fill;
        update(pad, padlen);
        uint8_t len[8];
        for (int i = 0; i < 8; i++) len[i] = (uint8_t)(bits >> (56 - 8 * i));
        update(len, 8);
        for (int i = 0; i < 8; i++) { out[4 * i] = (uint8_t)(h[i] >> 24); out[4 * i + 1] = (uint8_t)(h[i] >> 16); out[4 * i + 2] = (uint8_t)(h[i] >> 8); out[4 * i + 3] = (uint8_t)h[i]; }
    }
};
constexpr uint32_t Sha256Native::K_[64];
constexpr uint32_t Sha256Native::H0[8];

// 256-bit little-endian unsigned integers as 8 x u32 (digests read as BigUint::from_bytes_le)
struct U256 { uint32_t l[8]; };
U256 u256_from_le_bytes(const uint8_t b[32]) {
    U256 r;
    for (int i = 0; i < 8; i++) r.l[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
    return r;
}
// num / d, num % d for a divisor below 2^32 (get_mod_vals with the <= 20-bit moduli of this circuit)
void u256_divmod_small(const U256 &num, uint32_t d, U256 &q, uint32_t &rem) {
    uint64_t r = 0;
    for (int i = 7; i >= 0; i--) {
        const uint64_t cur = (r << 32) | num.l[i];
        q.l[i] = (uint32_t)(cur / d);
        r = cur % d;
    }
    rem = (uint32_t)r;
}
// Fr::from(BigUint) / Fr::from_le_bytes_mod_order for a 256-bit value: reduce mod r (2^256 < 3r), then to Montgomery form
Fr fr_from_u256(const U256 &v) {
    Fr c;
    for (int i = 0; i < 8; i++) c.l[i] = v.l[i];
    for (int k = 0; k < 3; k++) {
        bool ge = true;
        for (int i = 7; i >= 0; i--) {
            if (c.l[i] != FrP::mod(i)) { ge = c.l[i] > FrP::mod(i); break; }
        }
        if (!ge) break;
        uint32_t borrow = 0;
        for (int i = 0; i < 8; i++) {
            const uint64_t t = (uint64_t)c.l[i] - FrP::mod(i) - borrow;
            c.l[i] = (uint32_t)t;
            borrow = (uint32_t)(t >> 63);
        }
    }
    return fp_to_mont(c);
}
// into_bigint().to_bytes_le() of an Fr element: 32 bytes
void fr_to_le_bytes(const Fr &m, uint8_t out[32]) {
    const Fr c = fp_from_mont(m);
    for (int i = 0; i < 8; i++) { out[4 * i] = (uint8_t)c.l[i]; out[4 * i + 1] = (uint8_t)(c.l[i] >> 8); out[4 * i + 2] = (uint8_t)(c.l[i] >> 16); out[4 * i + 3] = (uint8_t)(c.l[i] >> 24); }
}
uint64_t modpow_u64(uint64_t b, uint64_t e, uint64_t m) {
    if (m == 1) return 0;
    uint64_t r = 1;
    b %= m;
    while (e) {
        if (e & 1) r = (unsigned __int128)r * b % m;
        b = (unsigned __int128)b * b % m;
        e >>= 1;
    }
    return r;
}

static const int PRIME_K = 3, PRIME_NUM_BITS = 20;

// check_if_next_is_prime (prime_circut.rs:165-195) + what PrimeCircuit::new needs
struct PrimeCandidate {
    uint8_t x_plus_j[32], digest[32], r_bytes[32];
    U256 digest_int, q;              // a_j = q * 2^20 + n
    uint32_t n = 0;                  // the 20-bit number tested
    Fr a;                            // the randomness r as a field element
    uint32_t base[PRIME_K];          // hashed Fermat bases mod n
    U256 base_int[PRIME_K], base_q[PRIME_K];
    bool is_prime = false;
};
// hash(r || j) mod n for j < K (hasher.rs:50-75: generate_bases_native)
void prime_bases(const Fr &a, uint32_t n, U256 base_int[PRIME_K], U256 base_q[PRIME_K], uint32_t base[PRIME_K]) {
    uint8_t ab[32], jb[32], dg[32];
    fr_to_le_bytes(a, ab);
    for (int j = 0; j < PRIME_K; j++) {
        fr_to_le_bytes(fr_from_u64((uint64_t)j), jb);
        Sha256Native s;
        s.update(ab, 32);
        s.update(jb, 32);
        s.finalize(dg);
        base_int[j] = u256_from_le_bytes(dg);
        u256_divmod_small(base_int[j], n, base_q[j], base[j]);
    }
}
PrimeCandidate prime_candidate(uint64_t x, uint64_t j) {
    PrimeCandidate c;
    const Fr xpj = fp_add(fr_from_u64(x), fr_from_u64(j));
    fr_to_le_bytes(xpj, c.x_plus_j);
    { Sha256Native s; s.update(c.x_plus_j, 32); s.finalize(c.digest); }
    c.digest_int = u256_from_le_bytes(c.digest);
    {   // r = hash(x + j || a_j || j)   (init_randomness, prime_circut.rs:148-158)
        Sha256Native s;
        uint8_t jl[8];
        for (int i = 0; i < 8; i++) jl[i] = (uint8_t)(j >> (8 * i));
        s.update(c.x_plus_j, 32); s.update(c.digest, 32); s.update(jl, 8);
        s.finalize(c.r_bytes);
    }
    c.a = fr_from_u256(u256_from_le_bytes(c.r_bytes));
    u256_divmod_small(c.digest_int, 1u << PRIME_NUM_BITS, c.q, c.n);
    if (c.n >= 2) {
        prime_bases(c.a, c.n, c.base_int, c.base_q, c.base);
        for (int k = 0; k < PRIME_K; k++)
            if (modpow_u64(c.base[k], c.n - 1, c.n) == 1) c.is_prime = true;      // fermat_test: any base passes
    }
    return c;
}

// the candidates zkg16_circuit_prime refuses (the reference panics on them) — every entry that takes (x, j) asks this one function
int prime_guard(const PrimeCandidate &c) {
    if (c.n < 2) return ZKG16_ERR_UNSUPPORTED;          // the reference's BigUint modpow panics on a modulus below 2
    for (int k = 0; k < PRIME_K; k++)
        if (c.base[k] == 0) return ZKG16_ERR_UNSUPPORTED;  // base.inverse().unwrap() panics upstream
    return ZKG16_OK;
}

// ------------------------------------------------------------------------------------------------ Boolean gadget
// ark_r1cs_std::boolean::Boolean: Constant(b) | Is(var) | Not(var)
struct Bit {
    enum Kind : uint8_t { CONST, IS, NOT } kind = CONST;
    VarId v = 0;
    bool val = false;
    static Bit constant(bool b) { Bit r; r.kind = CONST; r.val = b; return r; }
    Bit operator!() const {
        Bit r = *this;
        r.val = !val;
        if (kind == IS) r.kind = NOT; else if (kind == NOT) r.kind = IS;
        return r;
    }
};
// The recorder of the witness program (prime_program.hpp): attached, thread-local, only to the one recording build of a process —
// every hook below is a no-op otherwise, so ordinary builds are unchanged.  Indices are witness indices of that build's single
// segment; an operand that is not a witness bit marks the recording bad (the program is then refused, never used).
struct PrimeRecorder {
    struct Tag { uint32_t op = 0, a = 0, b = 0; uint64_t k = 0; };     // op 0: a slot; PRIME_SUM_MORE: a later result bit of a SUM
    static constexpr uint32_t PRIME_SUM_MORE = 5;
    std::vector<Tag> tag;
    std::vector<uint64_t> terms;              // SUM terms: witness index << 32 | shift | negated << 5
    std::vector<Fr> sources;                  // the values to_bits_le decomposed, in call order (Montgomery)
    std::vector<size_t> exp_rows;             // rows of check_bits_is_exp (A's column 0 holds n)
    size_t pack_row = SIZE_MAX;               // the packing row of to_bits_le(x + j) (C's column 0 holds -j)
    int part = 0;
    bool bad = false;
    void set(VarId v, uint32_t op, uint32_t a, uint32_t b, uint64_t k = 0) {
        if (!(v & WIT)) { bad = true; return; }
        const size_t w = v & ~WIT;
        if (tag.size() <= w) tag.resize(w + 1);
        tag[w] = Tag{op, a, b, k};
    }
    uint32_t operand(const Bit &b) {
        if (b.kind == Bit::CONST || !(b.v & WIT)) { bad = true; return 0; }
        return (b.v & ~WIT) | (b.kind == Bit::NOT ? PRIME_NEG : 0u);
    }
};
static thread_local PrimeRecorder *g_prime_rec = nullptr;

struct PrimeBuilder {
    Circuit &cs;
    const Fr one = Fr::one(), minus_one = fp_neg(Fr::one());
    explicit PrimeBuilder(Circuit &c) : cs(c) {}

    // rows are kept sorted by variable id with equal ids merged and zero coefficients dropped (ark's make_row)
    static void normalise(std::vector<Term> &t) {
        std::sort(t.begin(), t.end(), [](const Term &a, const Term &b) { return a.v < b.v; });
        size_t o = 0;
        for (size_t i = 0; i < t.size();) {
            Term acc = t[i++];
            while (i < t.size() && t[i].v == acc.v) acc.c = fp_add(acc.c, t[i++].c);
            if (!acc.c.is_zero()) t[o++] = acc;
        }
        t.resize(o);
    }
    // The 338 k rows of the circuit are mostly one to three terms long: they travel as spans over the caller's brace list or a
    // two-term stack value and are normalised in a small stack array — no heap traffic per row (the first version built three
    // std::vector per row and one per allocated variable: 47 ms of a 77 ms request, most of it in malloc / free).
    struct Span {
        const Term *p;
        size_t n;
        Span(std::initializer_list<Term> l) : p(l.begin()), n(l.size()) {}
        Span(const std::vector<Term> &v) : p(v.data()), n(v.size()) {}
        Span(const Term *p_, size_t n_) : p(p_), n(n_) {}
    };
    struct Terms2 {      // the linear form of one Boolean: at most One and the variable
        Term t[2];
        size_t n = 0;
        operator Span() const { return Span(t, n); }
    };
    std::vector<Term> scratch;
    void push_norm(int m, Span s) {
        if (s.n <= 4) {
            Term a[4];
            size_t k = 0;
            for (size_t i = 0; i < s.n; i++) {      // insertion sort by id, merging equal ids
                const Term &x = s.p[i];
                size_t pos = k;
                while (pos > 0 && a[pos - 1].v > x.v) pos--;
                if (pos > 0 && a[pos - 1].v == x.v) { a[pos - 1].c = fp_add(a[pos - 1].c, x.c); continue; }
                for (size_t q = k; q > pos; q--) a[q] = a[q - 1];
                a[pos] = x;
                k++;
            }
            size_t o = 0;
            for (size_t i = 0; i < k; i++)
                if (!a[i].c.is_zero()) a[o++] = a[i];
            cs.rows[m].push(a, o);
            return;
        }
        scratch.assign(s.p, s.p + s.n);
        normalise(scratch);
        cs.rows[m].push(scratch.data(), scratch.size());
    }
    void row(Span a, Span b, Span c) { push_norm(0, a); push_norm(1, b); push_norm(2, c); }
    // coeff * bit as terms
    void push_bit(std::vector<Term> &t, const Bit &b, const Fr &coeff) const {
        if (b.kind == Bit::CONST) { if (b.val) t.push_back(Term{0, coeff}); }
        else if (b.kind == Bit::IS) t.push_back(Term{b.v, coeff});
        else { t.push_back(Term{0, coeff}); t.push_back(Term{b.v, fp_neg(coeff)}); }
    }
    Terms2 bit_lc(const Bit &b) const {
        Terms2 r;
        if (b.kind == Bit::CONST) { if (b.val) r.t[r.n++] = Term{0, one}; }
        else if (b.kind == Bit::IS) r.t[r.n++] = Term{b.v, one};
        else { r.t[r.n++] = Term{0, one}; r.t[r.n++] = Term{b.v, minus_one}; }
        return r;
    }
    Bit alloc(bool v, bool input = false) {            // AllocatedBool: (1 - b) * b = 0
        Bit r;
        r.kind = Bit::IS;
        r.val = v;
        r.v = input ? cs.new_input_id(v ? one : Fr::zero()) : cs.new_witness_id(v ? one : Fr::zero());
        row({Term{0, one}, Term{r.v, minus_one}}, {Term{r.v, one}}, {});
        return r;
    }
    Bit raw(bool v, const Bit &a, const Bit &b, uint32_t op) {        // helper: fresh result variable without the booleanity row
        Bit r;
        r.kind = Bit::IS;
        r.val = v;
        r.v = cs.new_witness_id(v ? one : Fr::zero());
        if (g_prime_rec) {
            const uint32_t oa = g_prime_rec->operand(a), ob = g_prime_rec->operand(b);
            if (op == PRIME_OP_XOR && ((oa | ob) & PRIME_NEG)) g_prime_rec->bad = true;
            g_prime_rec->set(r.v, op, oa, ob);
        }
        return r;
    }
    Bit bxor(const Bit &a, const Bit &b) {
        if (a.kind == Bit::CONST) return a.val ? !b : b;
        if (b.kind == Bit::CONST) return b.val ? !a : a;
        if (a.kind == Bit::NOT && b.kind == Bit::NOT) return bxor(!a, !b);
        if (a.kind == Bit::NOT) return !bxor(!a, b);
        if (b.kind == Bit::NOT) return !bxor(a, !b);
        // AllocatedBool::xor: (a + a) * b = a + b - c
        const Bit c = raw(a.val != b.val, a, b, PRIME_OP_XOR);
        row({Term{a.v, fp_add(one, one)}}, {Term{b.v, one}}, {Term{a.v, one}, Term{b.v, one}, Term{c.v, minus_one}});
        return c;
    }
    Bit band(const Bit &a, const Bit &b) {
        if (a.kind == Bit::CONST) return a.val ? b : Bit::constant(false);
        if (b.kind == Bit::CONST) return b.val ? a : Bit::constant(false);
        // AllocatedBool::and / and_not / nor: one product row over the operands' linear forms
        const Bit c = raw(a.val && b.val, a, b, PRIME_OP_AND);
        row(bit_lc(a), bit_lc(b), {Term{c.v, one}});
        return c;
    }
    Bit bor(const Bit &a, const Bit &b) { return !band(!a, !b); }
    Bit kary_and(const std::vector<Bit> &v) {
        Bit cur = v[0];
        for (size_t i = 1; i < v.size(); i++) cur = band(cur, v[i]);
        return cur;
    }
    void enforce_nand2(const Bit &a, const Bit &b) {     // enforce_kary_nand(&[a, b]): nand == 1
        const Bit n = !band(a, b);
        if (n.kind == Bit::CONST) return;
        row(bit_lc(n), {Term{0, one}}, {Term{0, one}});
    }
    void enforce_equal(const Bit &a, const Bit &b) {     // Boolean::enforce_equal: (a - b) * 1 = 0
        if (a.kind == Bit::CONST && b.kind == Bit::CONST) return;
        const Terms2 la = bit_lc(a);
        std::vector<Term> d(la.t, la.t + la.n);
        push_bit(d, b, minus_one);
        row(d, {Term{0, one}}, {});
    }

    // ---- FpVar (linear combination + value) helpers on top of Circuit
    Lc lc_of(const std::vector<Term> &t, const Fr &val) const {
        Lc r;
        r.t = t;
        normalise(r.t);
        r.val = val;
        r.is_const = false;
        return r;
    }
    // AllocatedFp::to_bits_le: 255 Boolean witnesses (little-endian), one packing row, then enforce_in_field_le
    std::vector<Bit> to_bits_le(const Lc &x) {
        const Fr canon = fp_from_mont(x.val);
        std::vector<Bit> bits(255);
        for (int i = 0; i < 255; i++) bits[i] = alloc((canon.l[i >> 5] >> (i & 31)) & 1u);
        if (g_prime_rec) {
            for (int i = 0; i < 255; i++) g_prime_rec->set(bits[i].v, PRIME_OP_BITS, (uint32_t)g_prime_rec->sources.size(), (uint32_t)i);
            g_prime_rec->sources.push_back(x.val);
            if (g_prime_rec->part == 0 && g_prime_rec->pack_row == SIZE_MAX) g_prime_rec->pack_row = cs.rows[2].size();
        }
        std::vector<Term> lc;
        Fr coeff = one;
        for (int i = 0; i < 255; i++) { push_bit(lc, bits[i], coeff); coeff = fp_add(coeff, coeff); }
        for (const Term &t : x.t) lc.push_back(Term{t.v, fp_neg(t.c)});
        row({}, {}, lc);
        enforce_in_field_le(bits);
        return bits;
    }
    // Boolean::enforce_in_field_le = enforce_smaller_or_equal_than_le(bits, r - 1): runs of ones of r - 1 are AND-ed into
    // `last_run`; at every zero bit of r - 1 the value's bit and last_run must not both be set
    void enforce_in_field_le(const std::vector<Bit> &bits) {
        uint32_t pm1[8];
        for (int i = 0; i < 8; i++) pm1[i] = FrP::mod(i);
        pm1[0] -= 1;                                     // r is odd
        Bit last_run = Bit::constant(true);
        std::vector<Bit> current_run;
        for (int i = 254; i >= 0; i--) {
            const bool b = (pm1[i >> 5] >> (i & 31)) & 1u;
            const Bit &a = bits[i];
            if (b) {
                current_run.push_back(a);
            } else {
                if (!current_run.empty()) {
                    current_run.push_back(last_run);
                    last_run = kary_and(current_run);
                    current_run.clear();
                }
                enforce_nand2(last_run, a);
            }
        }
    }
    // AllocatedFp::to_bytes: to_bits_le padded with constant false to 256 bits, 8 per byte
    std::vector<Bit> to_bytes_bits(const Lc &x) {
        std::vector<Bit> b = to_bits_le(x);
        b.push_back(Bit::constant(false));
        return b;                                       // bit 8*k + t = bit t (little-endian) of byte k
    }
    static std::vector<Bit> constant_bytes_bits(const uint8_t *bytes, size_t n) {
        std::vector<Bit> b(8 * n);
        for (size_t i = 0; i < 8 * n; i++) b[i] = Bit::constant((bytes[i >> 3] >> (i & 7)) & 1);
        return b;
    }
    // FpVar::is_cmp_unchecked(self, other, Less, false) = ((self - other).double()).to_bits_le()[0]
    Bit is_smaller_than_unchecked(const Lc &a, const Lc &b) {
        const Lc d = Circuit::sub(a, b);
        return to_bits_le(Circuit::add(d, d))[0];
    }
    // AllocatedFp::is_eq = !is_neq: witnesses is_not_equal (Boolean) and multiplier; (a - b) * multiplier = is_not_equal,
    // (a - b) * (1 - is_not_equal) = 0
    Bit is_eq(const Lc &a, const Lc &b) {
        const Lc d = Circuit::sub(a, b);
        const bool neq = !d.val.is_zero();
        const Bit is_neq = alloc(neq);
        const Lc mult = cs.new_witness(neq ? fp_inv(d.val) : one);
        row(d.t, mult.t, {Term{is_neq.v, one}});
        row(d.t, {Term{0, one}, Term{is_neq.v, minus_one}}, {});
        return !is_neq;
    }
    // FpVar::inverse: inverse witness with self * inverse = 1
    Lc inverse(const Lc &a) {
        const Lc inv = cs.new_witness(fp_inv(a.val));
        cs.mul_equals(a, inv, cs.constant(one));
        return inv;
    }

    // ---- UInt32 as 32 little-endian Booleans
    struct U32 { Bit b[32]; };
    static U32 u32_const(uint32_t v) { U32 r; for (int i = 0; i < 32; i++) r.b[i] = Bit::constant((v >> i) & 1u); return r; }
    static uint32_t u32_val(const U32 &x) { uint32_t v = 0; for (int i = 0; i < 32; i++) v |= (uint32_t)x.b[i].val << i; return v; }
    static U32 rotr(const U32 &x, int n) { U32 r; for (int i = 0; i < 32; i++) r.b[i] = x.b[(i + n) & 31]; return r; }
    static U32 shr(const U32 &x, int n) { U32 r; for (int i = 0; i < 32; i++) r.b[i] = i + n < 32 ? x.b[i + n] : Bit::constant(false); return r; }
    U32 xor32(const U32 &a, const U32 &b) { U32 r; for (int i = 0; i < 32; i++) r.b[i] = bxor(a.b[i], b.b[i]); return r; }
    U32 and32(const U32 &a, const U32 &b) { U32 r; for (int i = 0; i < 32; i++) r.b[i] = band(a.b[i], b.b[i]); return r; }
    static U32 not32(const U32 &a) { U32 r; for (int i = 0; i < 32; i++) r.b[i] = !a.b[i]; return r; }
    // UInt32::addmany: result bits (32 + carry bits for the largest possible sum) allocated as Booleans, one row: sum - result = 0
    U32 addmany(const std::vector<U32> &ops) {
        bool all_const = true;
        uint64_t value = 0, max_value = 0;
        std::vector<Term> lc;
        for (const U32 &op : ops) {
            max_value += 0xffffffffull;
            value += u32_val(op);
            Fr coeff = one;
            for (int i = 0; i < 32; i++) {
                if (op.b[i].kind != Bit::CONST) all_const = false;
                push_bit(lc, op.b[i], coeff);
                coeff = fp_add(coeff, coeff);
            }
        }
        if (all_const) return u32_const((uint32_t)value);
        uint64_t rec_const = 0;
        const size_t rec_t0 = g_prime_rec ? g_prime_rec->terms.size() : 0;
        if (g_prime_rec)          // the sum as constant + (+-) bits << shift: a Not bit is 1 - b
            for (const U32 &op : ops)
                for (int s = 0; s < 32; s++) {
                    const Bit &b = op.b[s];
                    if (b.kind == Bit::CONST) { rec_const += (uint64_t)b.val << s; continue; }
                    if (b.kind == Bit::NOT) rec_const += 1ull << s;
                    g_prime_rec->terms.push_back((uint64_t)(b.v & ~WIT) << 32 | (uint64_t)s | (b.kind == Bit::NOT ? 32u : 0u));
                    if (!(b.v & WIT)) g_prime_rec->bad = true;
                }
        U32 res;
        Fr coeff = one;
        int i = 0;
        VarId first = 0;
        while (max_value != 0) {
            const Bit b = alloc((value >> i) & 1ull);
            if (g_prime_rec) {
                if (i == 0) first = b.v;
                else if (b.v != first + (VarId)i) g_prime_rec->bad = true;          // result bits are consecutive
                g_prime_rec->set(b.v, PrimeRecorder::PRIME_SUM_MORE, 0, 0);
            }
            lc.push_back(Term{b.v, fp_neg(coeff)});
            if (i < 32) res.b[i] = b;
            max_value >>= 1;
            i++;
            coeff = fp_add(coeff, coeff);
        }
        if (g_prime_rec) {
            const size_t nt = g_prime_rec->terms.size() - rec_t0;
            if (nt > 255 || i > 64) g_prime_rec->bad = true;                        // the instruction's 8-bit fields
            g_prime_rec->set(first, PRIME_OP_SUM, (uint32_t)rec_t0, (uint32_t)nt | (uint32_t)i << 8, rec_const);
        }
        row({}, {}, lc);
        return res;
    }

    // ---- Sha256Gadget: update over whole 64-byte blocks of little-endian byte bits, digest as 256 byte bits
    struct ShaState { U32 h[8]; };
    ShaState sha_init() { ShaState s; for (int i = 0; i < 8; i++) s.h[i] = u32_const(Sha256Native::H0[i]); return s; }
    // data: 64 bytes as 512 bits (bit 8*k + t = bit t of byte k); words are big-endian
    void sha_block(ShaState &st, const Bit *data) {
        std::vector<U32> w(64);
        for (int i = 0; i < 16; i++)
            for (int j = 0; j < 32; j++) w[i].b[j] = data[8 * (4 * i + 3 - (j >> 3)) + (j & 7)];
        for (int i = 16; i < 64; i++) {
            const U32 s0 = xor32(xor32(rotr(w[i - 15], 7), rotr(w[i - 15], 18)), shr(w[i - 15], 3));
            const U32 s1 = xor32(xor32(rotr(w[i - 2], 17), rotr(w[i - 2], 19)), shr(w[i - 2], 10));
            w[i] = addmany({w[i - 16], s0, w[i - 7], s1});
        }
        U32 h[8];
        for (int i = 0; i < 8; i++) h[i] = st.h[i];
        for (int i = 0; i < 64; i++) {
            const U32 ch = xor32(and32(h[4], h[5]), and32(not32(h[4]), h[6]));
            const U32 ma = xor32(xor32(and32(h[0], h[1]), and32(h[0], h[2])), and32(h[1], h[2]));
            const U32 s0 = xor32(xor32(rotr(h[0], 2), rotr(h[0], 13)), rotr(h[0], 22));
            const U32 s1 = xor32(xor32(rotr(h[4], 6), rotr(h[4], 11)), rotr(h[4], 25));
            const U32 t0 = addmany({h[7], s1, ch, u32_const(Sha256Native::K_[i]), w[i]});
            const U32 t1 = addmany({s0, ma});
            h[7] = h[6]; h[6] = h[5]; h[5] = h[4];
            h[4] = addmany({h[3], t0});
            h[3] = h[2]; h[2] = h[1]; h[1] = h[0];
            h[0] = addmany({t0, t1});
        }
        for (int i = 0; i < 8; i++) st.h[i] = addmany({st.h[i], h[i]});
    }
    // whole message (byte bits) -> digest byte bits (32 bytes, big-endian words)
    std::vector<Bit> sha256(const std::vector<Bit> &msg_bits) {
        const size_t nbytes = msg_bits.size() / 8;
        std::vector<Bit> padded = msg_bits;
        auto push_byte = [&](uint8_t v) { for (int t = 0; t < 8; t++) padded.push_back(Bit::constant((v >> t) & 1)); };
        push_byte(0x80);
        while ((padded.size() / 8) % 64 != 56) push_byte(0);
        const uint64_t bitlen = (uint64_t)nbytes * 8;
        for (int i = 0; i < 8; i++) push_byte((uint8_t)(bitlen >> (56 - 8 * i)));
        ShaState st = sha_init();
        for (size_t off = 0; off < padded.size(); off += 512) sha_block(st, padded.data() + off);
        std::vector<Bit> out(256);
        for (int i = 0; i < 8; i++)
            for (int k = 0; k < 4; k++)                      // byte k of word i = bits 8*(3-k) .. of the word
                for (int t = 0; t < 8; t++) out[8 * (4 * i + k) + t] = st.h[i].b[8 * (3 - k) + t];
        return out;
    }
    static void bits_to_bytes(const std::vector<Bit> &bits, uint8_t *out) {
        for (size_t k = 0; k < bits.size() / 8; k++) {
            uint8_t v = 0;
            for (int t = 0; t < 8; t++) v |= (uint8_t)bits[8 * k + t].val << t;
            out[k] = v;
        }
    }
};

// mod_pow_generate_witnesses (modulo.rs:31-89) for the 20-bit moduli of this circuit: per step the quotient / remainder of the
// running product and of the running square
struct ModpowTrace {
    uint64_t res_q[PRIME_NUM_BITS], res_rem[PRIME_NUM_BITS], pow_q[PRIME_NUM_BITS], pow_rem[PRIME_NUM_BITS];
    uint32_t bits[PRIME_NUM_BITS];
    uint64_t result;
};
ModpowTrace modpow_trace(uint64_t base, uint64_t div, uint64_t exp) {
    ModpowTrace t;
    memset(&t, 0, sizeof t);
    uint64_t power = base;
    for (int i = 0; i < PRIME_NUM_BITS; i++) {        // squares: power = power^2, (q, rem) of it, power %= div
        power = power * power;
        t.pow_q[i] = power / div;
        t.pow_rem[i] = power % div;
        power %= div;
    }
    uint64_t cur_pow = base, res = 1, e = exp;
    int counter = 0;
    while (e > 0 && counter < PRIME_NUM_BITS) {
        const uint64_t elem = e & 1;
        t.bits[counter] = (uint32_t)elem;
        res *= (cur_pow - 1) * elem + 1;
        t.res_q[counter] = res / div;
        t.res_rem[counter] = res % div;
        if (res > div) res %= div;
        e >>= 1;
        cur_pow = cur_pow * cur_pow % div;
        counter++;
    }
    for (int i = counter; i < PRIME_NUM_BITS; i++) { t.res_q[i] = 0; t.res_rem[i] = res; }
    t.result = res;
    return t;
}

// PrimeCircuit::generate_constraints for the candidate found by the native search
// The circuit is built in seven parts whose rows follow each other in this order: [x, SHA-256(x + j), the digest inputs, the
// division by 2^20, n and a], [Fermat base k = 0, 1, 2: bytes of a, SHA-256(a || k), the witnessed remainder], [modpow k = 0, 1, 2].
// A part touches the others only through three kinds of variables (n, a, the three bases), so each can be built into its own
// Circuit segment on its own thread once it is known how many witnesses the parts before it allocate — which does not depend on
// (x, j): the first build of a process runs the parts one after another and records those counts (PrimeLayout).
static constexpr int PRIME_PARTS = 7;
struct PrimeShared {          // what later parts need of earlier ones: variable ids (values are known natively)
    VarId n = 0, a = 0, base[PRIME_K] = {0, 0, 0};
};
static Lc prime_var(VarId id, const Fr &val) {
    Lc r;
    r.t.push_back(Term{id, Fr::one()});
    r.val = val;
    r.is_const = false;
    return r;
}

static void prime_part_head(Circuit &cs, uint64_t x, uint64_t j, const PrimeCandidate &c, PrimeShared &sh) {
    PrimeBuilder g(cs);
    // x (instance), x + i, hash(x + i)
    const Lc x_var = cs.new_input(fr_from_u64(x));
    Lc x_plus_i = x_var;
    Circuit::add_const(x_plus_i, fr_from_u64(j));
    const std::vector<Bit> calc = g.sha256(g.to_bytes_bits(x_plus_i));
    // a_i: 32 bytes as instance Booleans (DigestVar::new_input), equal to the computed digest
    std::vector<Bit> a_i(256);
    for (int k = 0; k < 256; k++) a_i[k] = g.alloc((c.digest[k >> 3] >> (k & 7)) & 1, true);
    for (int k = 0; k < 256; k++) g.enforce_equal(a_i[k], calc[k]);
    // a_i as a field element; div = 2^20, origin, remainder, quotient: div * quotient + remainder = origin = a_i
    const Fr a_i_fr = fr_from_u256(c.digest_int);
    const Lc a_i_fp = cs.new_witness(a_i_fr);
    const Lc div = cs.new_witness(fr_from_u64(1ull << PRIME_NUM_BITS));
    const Lc origin = cs.new_witness(a_i_fr);
    const Lc remainder = cs.new_witness(fr_from_u64(c.n));
    const Lc quotient = cs.new_witness(fr_from_u256(c.q));
    cs.enforce_equal(Circuit::add(cs.mul(div, quotient), remainder), origin);
    cs.enforce_equal(origin, a_i_fp);
    const Lc n_var_fermat = cs.new_witness(fr_from_u64(c.n));
    cs.enforce_equal(n_var_fermat, remainder);
    // ---- FermatCircuit (fermat_circut.rs:104-130)
    const Lc n = cs.new_witness(fr_from_u64(c.n));
    const Lc a = cs.new_witness(c.a);
    sh.n = n.t[0].v;
    sh.a = a.t[0].v;
}

// generate_bases_a (hasher.rs:77-111): base_k = hash(a || k) mod n with witnessed quotient
static void prime_part_base(Circuit &cs, int k, const PrimeCandidate &c, PrimeShared &sh) {
    PrimeBuilder g(cs);
    const Lc a = prime_var(sh.a, c.a);
    std::vector<Bit> msg = g.to_bytes_bits(a);
    uint8_t jb[32];
    fr_to_le_bytes(fr_from_u64((uint64_t)k), jb);
    const std::vector<Bit> jbits = PrimeBuilder::constant_bytes_bits(jb, 32);
    msg.insert(msg.end(), jbits.begin(), jbits.end());
    const std::vector<Bit> dg = g.sha256(msg);
    (void)dg;                                         // the reference only reads its value (a fresh witness follows)
    const Lc a_j = cs.new_witness(fr_from_u256(c.base_int[k]));
    const Lc rem = cs.new_witness(fr_from_u64(c.base[k]));
    const Lc quo = cs.new_witness(fr_from_u256(c.base_q[k]));
    const Lc dv = cs.new_witness(fr_from_u64(c.n));
    cs.enforce_equal(Circuit::add(cs.mul(quo, dv), rem), a_j);
    sh.base[k] = rem.t[0].v;
}

static void prime_part_fermat(Circuit &cs, int k, const PrimeCandidate &c, const PrimeShared &sh) {
    PrimeBuilder g(cs);
    const Fr one = Fr::one();
    const Lc n = prime_var(sh.n, fr_from_u64(c.n));
    const Lc base = prime_var(sh.base[k], fr_from_u64(c.base[k]));
    const Lc one_c = cs.constant(one);
    const ModpowTrace tr = modpow_trace(c.base[k], c.n, c.n - 1);
    const Lc result = cs.new_witness(fr_from_u64(tr.result));
    const Bit is_prime = g.alloc(c.is_prime);
    const Lc other_res = cs.new_witness(fr_from_u64(tr.result));
    cs.enforce_equal(result, other_res);
    Lc n_minus_one = n;
    Circuit::add_const(n_minus_one, fp_neg(one));
    // modpow (fermat_circut.rs:56-101)
    {
        Lc cur_pow = base;
        const Lc result2 = cs.new_witness(fr_from_u64(tr.result));
        const Lc one_v = cs.mul(base, g.inverse(base));       // `one` is a variable: base * base^-1
        Lc calculated = one_v;
        {   // check_bits_is_exp: a zero witness plus the exponent's bits as constants must equal n - 1
            Lc res = cs.new_witness(Fr::zero());
            uint64_t e = 0;
            for (int i = 0; i < PRIME_NUM_BITS; i++) e |= (uint64_t)tr.bits[i] << i;
            Circuit::add_const(res, fr_from_u64(e));
            if (g_prime_rec) g_prime_rec->exp_rows.push_back(cs.rows[0].size());
            cs.enforce_equal(res, n_minus_one);
        }
        for (int i = 0; i < PRIME_NUM_BITS; i++) {
            const Lc elem = cs.new_witness(fr_from_u64(tr.bits[i]));
            const Lc factor = Circuit::add(cs.mul(elem, Circuit::sub(cur_pow, one_v)), one_v);
            calculated = cs.mul(calculated, factor);
            const Lc q1 = cs.new_witness(fr_from_u64(tr.res_q[i]));
            const Lc r1 = cs.new_witness(fr_from_u64(tr.res_rem[i]));
            cs.enforce_equal(Circuit::add(cs.mul(q1, n), r1), calculated);
            (void)g.is_smaller_than_unchecked(r1, n);          // computed and ignored by the reference
            calculated = r1;
            cur_pow = cs.mul(cur_pow, cur_pow);
            const Lc q2 = cs.new_witness(fr_from_u64(tr.pow_q[i]));
            const Lc r2 = cs.new_witness(fr_from_u64(tr.pow_rem[i]));
            cs.enforce_equal(Circuit::add(cs.mul(q2, n), r2), cur_pow);
            (void)g.is_smaller_than_unchecked(r2, n);
            cur_pow = r2;
        }
        cs.enforce_equal(calculated, result2);
    }
    // result.is_eq(1) == is_prime
    const Bit eq = g.is_eq(result, one_c);
    g.enforce_equal(eq, is_prime);
}

// part p into cs (the one circuit of the sequential build, or the part's own segment)
static void prime_part(Circuit &cs, int p, uint64_t x, uint64_t j, const PrimeCandidate &c, PrimeShared &sh) {
    if (p == 0) prime_part_head(cs, x, j, c, sh);
    else if (p <= PRIME_K) prime_part_base(cs, p - 1, c, sh);
    else prime_part_fermat(cs, p - 1 - PRIME_K, c, sh);
}

// witnesses allocated before each part (and in total) + the shared variable ids: recorded by the first sequential build
struct PrimeLayout {
    bool known = false;
    size_t wit_base[PRIME_PARTS + 1] = {0};
    size_t rows_hint[PRIME_PARTS] = {0}, nnz_hint[PRIME_PARTS][3] = {{0}};
    PrimeShared sh;
};

// the whole circuit into ONE Circuit, parts in order (the reference's order); fills `lay` when given
void build_prime_circuit(Circuit &cs, uint64_t x, uint64_t j, const PrimeCandidate &c, PrimeLayout *lay = nullptr) {
    // the circuit's size does not depend on (x, j): 338,296 rows, 320,687 witnesses, 465,904 / 336,259 / 731,820 non-zeros
    cs.witness.reserve(321000);
    const size_t nnz_hint[3] = {466000, 337000, 732000};
    for (int m = 0; m < 3; m++) { cs.rows[m].t.reserve(nnz_hint[m]); cs.rows[m].ptr.reserve(338400); }
    PrimeShared sh;
    for (int p = 0; p < PRIME_PARTS; p++) {
        if (lay) {
            lay->wit_base[p] = cs.witness.size();
            if (p > 0) {
                lay->rows_hint[p - 1] = cs.rows[0].size();
                for (int m = 0; m < 3; m++) lay->nnz_hint[p - 1][m] = cs.rows[m].t.size();
            }
        }
        if (g_prime_rec) g_prime_rec->part = p;
        prime_part(cs, p, x, j, c, sh);
    }
    if (lay) {
        lay->wit_base[PRIME_PARTS] = cs.witness.size();
        lay->rows_hint[PRIME_PARTS - 1] = cs.rows[0].size();
        for (int m = 0; m < 3; m++) lay->nnz_hint[PRIME_PARTS - 1][m] = cs.rows[m].t.size();
        for (int p = PRIME_PARTS - 1; p > 0; p--) {      // cumulative -> per part
            lay->rows_hint[p] -= lay->rows_hint[p - 1];
            for (int m = 0; m < 3; m++) lay->nnz_hint[p][m] -= lay->nnz_hint[p - 1][m];
        }
        lay->sh = sh;
        lay->known = true;
    }
}

// The values the witness program takes as inputs (prime_program.hpp), natively, in the order the builders above allocate them:
// the slots (every witness that is not a Boolean gadget result, in allocation order) and the sources (what to_bits_le decomposes,
// in call order).  Every step repeats the builders' own field operations on the same values; the recording build compares the
// result with what it allocated before the program is used (circuits.hip: prime_record).
static void prime_native_inputs(uint64_t x, uint64_t j, const PrimeCandidate &c, std::vector<Fr> &slot, std::vector<Fr> &src) {
    const Fr one = Fr::one(), zero = Fr::zero(), minus_one = fp_neg(Fr::one());
    auto sub = [&](const Fr &a, const Fr &b) { return fp_add(a, fp_mul(b, minus_one)); };          // Circuit::sub
    auto bit = [&](bool b) { return b ? one : zero; };
    const Fr fn = fr_from_u64(c.n);
    // head: to_bits_le(x + j); a_i, div, origin, remainder, quotient, div * quotient, n (twice more), a
    src.push_back(fp_add(fr_from_u64(x), fr_from_u64(j)));
    {
        const Fr a_i = fr_from_u256(c.digest_int), div = fr_from_u64(1ull << PRIME_NUM_BITS), q = fr_from_u256(c.q);
        for (const Fr &v : {a_i, div, a_i, fn, q, fp_mul(div, q), fn, fn, c.a}) slot.push_back(v);
    }
    // bases: to_bits_le(a); a_j, rem, quo, n, quo * n
    for (int k = 0; k < PRIME_K; k++) {
        src.push_back(c.a);
        const Fr quo = fr_from_u256(c.base_q[k]);
        for (const Fr &v : {fr_from_u256(c.base_int[k]), fr_from_u64(c.base[k]), quo, fn, fp_mul(quo, fn)}) slot.push_back(v);
    }
    // Fermat parts (prime_part_fermat)
    for (int k = 0; k < PRIME_K; k++) {
        const Fr base = fr_from_u64(c.base[k]);
        const ModpowTrace tr = modpow_trace(c.base[k], c.n, c.n - 1);
        const Fr result = fr_from_u64(tr.result);
        const Fr inv = fp_inv(base), one_v = fp_mul(base, inv);
        for (const Fr &v : {result, bit(c.is_prime), result, result, inv, one_v, zero}) slot.push_back(v);
        Fr cur_pow = base, calculated = one_v;
        for (int i = 0; i < PRIME_NUM_BITS; i++) {
            const Fr elem = fr_from_u64(tr.bits[i]);
            const Fr m = fp_mul(elem, sub(cur_pow, one_v));
            calculated = fp_mul(calculated, fp_add(m, one_v));
            const Fr q1 = fr_from_u64(tr.res_q[i]), r1 = fr_from_u64(tr.res_rem[i]);
            for (const Fr &v : {elem, m, calculated, q1, r1, fp_mul(q1, fn)}) slot.push_back(v);
            const Fr d1 = sub(r1, fn);
            src.push_back(fp_add(d1, d1));
            calculated = r1;
            cur_pow = fp_mul(cur_pow, cur_pow);
            const Fr q2 = fr_from_u64(tr.pow_q[i]), r2 = fr_from_u64(tr.pow_rem[i]);
            for (const Fr &v : {cur_pow, q2, r2, fp_mul(q2, fn)}) slot.push_back(v);
            const Fr d2 = sub(r2, fn);
            src.push_back(fp_add(d2, d2));
            cur_pow = r2;
        }
        const Fr d = sub(result, one);                                                      // is_eq(result, 1)
        const bool neq = !d.is_zero();
        slot.push_back(bit(neq));
        slot.push_back(neq ? fp_inv(d) : one);
    }
}
