// The PrimeCircuit as a recorded PROGRAM: what a kernel (prime_device.hip) or a plain loop (zkg16_prime_witness_host, the test
// reference) needs to write the circuit's assignment and R1CS for candidate (x, j) without synthesising 338 k constraints.
//
// The circuit's structure does not depend on (x, j) (prime_circuit.inc).  A sequential build, run once per process with a recorder
// attached, notes for every witness how its value arises:
//   - a Boolean gadget result: XOR / AND of two earlier bits (AND with optional negations), all result bits of one UInt32::addmany
//     (the bits of an integer sum of earlier bits), or bit t of a field value that to_bits_le decomposes;
//   - anything else (quotients, remainders, products, inverses, n, a, the flags is_prime / is_neq): a SLOT, a field element the host
//     computes natively per request (prime_inputs) next to the few values to_bits_le decomposes (SOURCES).
// Bits never depend on another part's bits (the parts touch only through n, a and the bases, which are slots), so each of the seven
// parts runs as one workgroup whose bits stay in LDS; its instructions are sorted by dependency level.
// The R1CS is the recorded one with four coefficients patched: A's column-0 coefficient n in the three check_bits_is_exp rows, and
// C's column-0 coefficient -j in the packing row of to_bits_le(x + j) — absent when j = 0 (that C matrix has one non-zero fewer).
#pragma once
#include <stdint.h>

#include <memory>
#include <vector>

#include "ff.cuh"

namespace zk {

static constexpr int PRIME_PROGRAM_PARTS = 7;
enum PrimeOp : uint32_t { PRIME_OP_XOR = 1, PRIME_OP_AND = 2, PRIME_OP_SUM = 3, PRIME_OP_BITS = 4 };
static constexpr uint32_t PRIME_SLOT = 0x80000000u;       // code[] entry: a slot (else the witness index of a bit)
static constexpr uint32_t PRIME_NEG = 0x80000000u;        // AND operand: negated
// one instruction (16 B).  op_dst = op << 29 | part-local destination.  Operands are part-local bit indices.
//   XOR  a, b                     AND  a | NEG?, b | NEG?                BITS a = source, b = bit position
//   SUM  a = first term, b = nterms | nbits << 8 | (constant >> 32) << 16, c = low 32 bits of the constant; writes nbits bits
//        (destination onward) of  constant + sum over terms of (+-) bit << shift.  Term: index | shift << 18 | negated << 23.
struct PrimeInstr { uint32_t op_dst, a, b, c; };

struct PrimeProgram {
    size_t num_instance = 0, num_witness = 0, num_constraints = 0;
    uint32_t wit_base[PRIME_PROGRAM_PARTS + 1] = {0};
    // ---- witness program
    std::vector<PrimeInstr> ins;                       // part by part, each sorted by level
    std::vector<uint32_t> lvl;                         // level L covers ins[lvl[L], lvl[L + 1]); part p: levels [lvl_base[p], lvl_base[p + 1])
    uint32_t lvl_base[PRIME_PROGRAM_PARTS + 1] = {0};
    uint32_t part_ins[PRIME_PROGRAM_PARTS] = {0};      // instructions per part (the report in DESIGN.md)
    std::vector<uint32_t> terms;
    std::vector<uint32_t> code;                        // per z entry: PRIME_SLOT | slot, or a witness index (its bit)
    size_t n_slots = 0, n_sources = 0;                 // slots include the instance (slot v = z[v] for v < num_instance)
    uint32_t max_part = 0;                             // witnesses of the largest part (bytes of LDS)
    // ---- R1CS template, in its j >= 1 form
    std::vector<uint64_t> rp[3];
    std::vector<uint32_t> col[3];
    std::vector<Fr> cf[3];
    std::vector<uint64_t> rp_c_j0;                     // C's row pointers when j = 0
    uint64_t a_pos[3] = {0, 0, 0}, c_pos = 0;          // the patched non-zeros
    uint32_t patch_rows[4] = {0, 0, 0, 0};             // ... and the constraint rows that hold them (A, A, A, C)
};

// one instruction on the bits of its part (LDS on the device, a host array in zkg16_prime_witness_host); src: canonical sources
ZK_HD void prime_exec(const PrimeInstr &in, uint8_t *bit, const uint32_t *terms, const Fr *src) {
    const uint32_t op = in.op_dst >> 29, d = in.op_dst & 0x1fffffffu;
    if (op == PRIME_OP_XOR) {
        bit[d] = bit[in.a] ^ bit[in.b];
    } else if (op == PRIME_OP_AND) {
        bit[d] = (bit[in.a & ~PRIME_NEG] ^ (uint8_t)(in.a >> 31)) & (bit[in.b & ~PRIME_NEG] ^ (uint8_t)(in.b >> 31));
    } else if (op == PRIME_OP_BITS) {
        bit[d] = (uint8_t)((src[in.a].l[in.b >> 5] >> (in.b & 31u)) & 1u);
    } else {                 // PRIME_OP_SUM: the true sum is non-negative; unsigned wrap-around in between is harmless
        const uint32_t nt = in.b & 255u, nb = (in.b >> 8) & 255u;
        uint64_t sum = (uint64_t)(in.b >> 16) << 32 | in.c;
        for (uint32_t k = 0; k < nt; k++) {
            const uint32_t t = terms[in.a + k];
            const uint64_t v = (uint64_t)bit[t & 0x3ffffu] << ((t >> 18) & 31u);
            sum = ((t >> 23) & 1u) ? sum - v : sum + v;
        }
        for (uint32_t i = 0; i < nb; i++) bit[d + i] = (uint8_t)((sum >> i) & 1u);
    }
}

// circuits.hip.  prime_program: the program, recorded by the first caller of a process (a sequential build of a valid candidate).
// prime_inputs: the slots (Montgomery) and sources (canonical) of candidate (x, j) — or ZKG16_ERR_UNSUPPORTED for the candidates
// zkg16_circuit_prime refuses.  Both return a zkg16_status.
int prime_program(std::shared_ptr<const PrimeProgram> &out);
int prime_inputs(const PrimeProgram &P, uint64_t x, uint64_t j, std::vector<Fr> &slots, std::vector<Fr> &sources, uint32_t *n_out);

}  // namespace zk
