/* kzg.h -- C++ API of the MI355X KZG engine, mirroring the reference's
 * public surface (/root/reference/src/kzg.h:27-292, namespace kzg) so a user
 * of uncommitted6453/kzg-commitments can switch by re-linking:
 *
 *   kzg::init                       src/kzg.h:38        trusted_setup.cpp:15-19
 *   kzg::blob::from_string/bytes    src/kzg.h:40-87     blob.cpp:3-48
 *   kzg::poly::from_blob/(de)ser.   src/kzg.h:89-125    poly.cpp:4-15, util.cpp:118-170
 *   kzg::commit / kzg::proof        src/kzg.h:127-180   commit.cpp, proof.cpp, util.cpp:78-115
 *   kzg::trusted_setup              src/kzg.h:182-290   trusted_setup.cpp:21-287
 *
 * Differences, all at the type level (semantics and error behaviour follow
 * the reference): NTL ZZ_p / ZZ_pX are replaced by kzg::Fr / std::vector<Fr>
 * (canonical residues mod r), miracl ECP by kzg::G1 (canonical affine
 * coordinates), and the curve is chosen at run time (kzg::init(curve))
 * instead of by rebuilding with another kzg_config.h.  Every group and
 * scalar-field computation runs on the GPU through the C ABI in kzg_gpu.h.
 */
#ifndef KZG_H
#define KZG_H

#include <array>
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "kzg_gpu.h"

namespace kzg {

extern int CURVE_ORDER_BYTES;

#define MAX_CHUNK_BYTES (kzg::CURVE_ORDER_BYTES - 1)

/** Element of Z_r (the reference's NTL ZZ_p under ZZ_p::init(r)). */
struct Fr {
  std::array<uint64_t, 4> v{};  // little-endian limbs, always < r
  Fr() = default;
  /** integer -> residue, like NTL `ZZ_p x; x = long` (negative -> r - |x|) */
  Fr(long x);
  /** little-endian bytes -> residue (NTL ZZFromBytes + conv<ZZ_p>) */
  static Fr from_le_bytes(const uint8_t* bytes, size_t n);
  /** minimal little-endian encoding (NTL BytesFromZZ with NumBytes) */
  std::vector<uint8_t> to_le_bytes() const;
  bool is_zero() const { return (v[0] | v[1] | v[2] | v[3]) == 0; }
  bool operator==(const Fr& o) const { return v == o.v; }
  bool operator!=(const Fr& o) const { return v != o.v; }
};

/** Affine G1 point (the reference's miracl ECP); canonical coordinates. */
struct G1 {
  std::array<uint64_t, 6> x{}, y{};  // 4 limbs used on BN254, 6 on BLS12-381
  bool inf = true;
  bool operator==(const G1& o) const { return inf == o.inf && (inf || (x == o.x && y == o.y)); }
  bool operator!=(const G1& o) const { return !(*this == o); }
};

/** Affine G2 point on the sextic twist (the reference's miracl ECP2):
 *  x = x0 + x1 i, y = y0 + y1 i, canonical coordinates. */
struct G2 {
  std::array<uint64_t, 6> x0{}, x1{}, y0{}, y1{};
  bool inf = true;
  bool operator==(const G2& o) const {
    return inf == o.inf && (inf || (x0 == o.x0 && x1 == o.x1 && y0 == o.y0 && y1 == o.y1));
  }
  bool operator!=(const G2& o) const { return !(*this == o); }
};

/** Initialize the library (BN254, the reference's default build). */
void init();
/** Extension: pick the curve at run time (KZGX_CURVE_BN254 / KZGX_CURVE_BLS12381). */
void init(int curve);
/** Curve selected by init(). */
int curve();
/** Extension: the GPU (HIP device ordinal) that trusted_setups constructed
 *  after this call, and the setup-independent polynomial helpers, run on
 *  (default 0).  One process per GPU is the multi-GPU model; a process may
 *  also hold setups on several devices.  @throws std::invalid_argument for a
 *  negative ordinal (a missing device fails at the next construction). */
void set_device(int device);
int device();
/** Extension: the generator w of the size-2^log2n domain {w^i} that the
 *  evaluation-form calls below work on (kzgx_domain_root): BLS12-381
 *  7^((r-1)/2^log2n), log2n <= 32; BN254 2^((r-1)/2^log2n), log2n <= 2.
 *  @throws std::invalid_argument beyond the field's 2-adicity */
Fr domain_root(unsigned log2n);

class blob {
 private:
  std::vector<std::pair<Fr, Fr>> data;

 public:
  blob(std::vector<std::pair<Fr, Fr>>& _data) : data(_data) {}
  std::vector<std::pair<Fr, Fr>>& get_data() { return data; }
  /** points (i + offset, (signed char) s[i]) (blob.cpp:7-18) */
  static blob from_string(std::string s);
  static blob from_string(std::string s, int offset);
  /** little-endian chunk_size-byte chunks; x = byte_offset / chunk_size + i (blob.cpp:20-48)
   *  @throws std::invalid_argument on chunk_size / alignment violations */
  static blob from_bytes(const uint8_t* bytes, int byte_offset, int byte_length, int chunk_size);
};

class poly {
 private:
  std::vector<Fr> data;  // normalized: no trailing zero coefficient

 public:
  poly(std::vector<Fr> _data);
  const std::vector<Fr>& get_poly() const { return data; }
  /** NTL deg(): -1 for the zero polynomial */
  long degree() const { return (long)data.size() - 1; }
  /** interpolate the blob's points (polyfit, util.cpp:172-184) on the GPU */
  static poly from_blob(blob blob);
  /** Extension: the polynomial of degree < evals.size() with P(w^i) = evals[i],
   *  w = domain_root(log2 size), by an inverse NTT on the GPU of device()
   *  (kzgx_ntt); bit_reversed: evals[bit reversal of i] holds P(w^i).
   *  Normalized as the constructor does.  BLS12-381 up to 2^22 values; BN254's
   *  scalar field has no domain beyond 4 (from_blob interpolates there).
   *  @throws std::invalid_argument if the size is not a power of two or
   *          exceeds the curve's domain */
  static poly from_evaluations(const std::vector<Fr>& evals, bool bit_reversed = false);
  /** Extension: P on the whole size-2^log2n domain (forward NTT of the
   *  zero-padded coefficients), element i = P(w^i), or with bit_reversed
   *  element (bit reversal of i).
   *  @throws std::invalid_argument if deg + 1 > 2^log2n or the size exceeds
   *          the curve's domain */
  std::vector<Fr> evaluate_domain(unsigned log2n, bool bit_reversed = false) const;
  std::vector<uint8_t> serialize();
  static poly deserialize(const std::vector<uint8_t>&);
};

class commit {
 private:
  G1 curve_point;

 public:
  commit(G1 _curve_point) : curve_point(_curve_point) {}
  G1& get_curve_point() { return curve_point; }
  std::vector<uint8_t> serialize();
  static commit deserialize(const std::vector<uint8_t>&);
  /** Extension: deserialize() of every entry with one GPU pass for the whole
   *  batch (kzgx_g1_check_batch; the host only parses octets).  Element k ==
   *  deserialize(bytes[k]) when check_subgroup is false: a malformed or
   *  off-curve octet decodes to infinity.  With check_subgroup a point outside
   *  the prime-order subgroup (BLS12-381) decodes to infinity too.  valid[k]:
   *  entry k was a well-formed point that passed the chosen checks. */
  static std::vector<commit> deserialize_batch(const std::vector<std::vector<uint8_t>>& bytes,
                                               bool check_subgroup = false, std::vector<bool>* valid = nullptr);
  /** Extension: the bare compressed record of kzg_gpu.h "compressed points"
   *  (KZGX_ENC_ZCASH: 48 bytes, BLS12-381 only; KZGX_ENC_SEC1: 1 + MODBYTES
   *  bytes, the compressed counterpart of serialize()'s 0x04 octet).  No u32
   *  length prefix: the formats are fixed-size.
   *  @throws std::invalid_argument for an encoding the curve does not offer */
  std::vector<uint8_t> serialize_compressed(int encoding);
  /** Extension: `packed` holds whole records of `encoding` back to back; one GPU
   *  pass decompresses (a square root per record) and checks them all
   *  (kzgx_g1_decompress_batch).  A record that is malformed, non-canonical,
   *  without a root or, with check_subgroup, outside the prime-order subgroup
   *  decodes to infinity with valid[k] = false; the identity record is valid.
   *  @throws std::invalid_argument for an encoding the curve does not offer or
   *          a size that is not a multiple of the record length */
  static std::vector<commit> deserialize_compressed_batch(const std::vector<uint8_t>& packed, int encoding,
                                                          bool check_subgroup = false,
                                                          std::vector<bool>* valid = nullptr);
};

class proof {
 private:
  G1 curve_point;

 public:
  proof(G1 _curve_point) : curve_point(_curve_point) {}
  G1& get_curve_point() { return curve_point; }
  std::vector<uint8_t> serialize();
  static proof deserialize(const std::vector<uint8_t>& bytes);
  /** Extension: as commit::deserialize_batch. */
  static std::vector<proof> deserialize_batch(const std::vector<std::vector<uint8_t>>& bytes,
                                              bool check_subgroup = false, std::vector<bool>* valid = nullptr);
  /** Extensions: as commit::serialize_compressed / deserialize_compressed_batch. */
  std::vector<uint8_t> serialize_compressed(int encoding);
  static std::vector<proof> deserialize_compressed_batch(const std::vector<uint8_t>& packed, int encoding,
                                                         bool check_subgroup = false,
                                                         std::vector<bool>* valid = nullptr);
};

/** Extension: one group of a batch opening (trusted_setup::create_batch_proofs):
 *  the polynomials (or, for the verifier, the commitments) named by `polys`,
 *  indices into the call's list, all opened at `point` under one proof. */
struct batch_opening {
  Fr point;
  std::vector<uint32_t> polys;
};

/** Extension: one opening set of a Shplonk opening (trusted_setup::create_shplonk_proof):
 *  `points` are indices into the call's list of points (no index twice),
 *  `polys` indices into its list of polynomials (or, for the verifier,
 *  commitments); every named polynomial is opened at every named point. */
struct shplonk_set {
  std::vector<uint32_t> points, polys;
};

/** Extension: a Shplonk proof -- two G1 points, whatever was opened. */
struct shplonk_proof {
  proof W, Wp;
};

class trusted_setup {
 private:
  kzgx_ctx* ctx = nullptr;  // device SRS + stream + workspaces
  size_t n = 0;

  trusted_setup() = default;  // from_compressed fills it in
  G1 polyeval_G1(const std::vector<Fr>& P);
  bool aggregated(std::vector<commit>& commits, std::vector<proof>& proofs,
                  const std::vector<std::pair<Fr, Fr>>& points, bool checked, bool check_subgroup);
  bool coset_aggregated(std::vector<commit>& commits, const std::vector<uint32_t>& commit_index,
                        const std::vector<uint32_t>& cell_index, std::vector<proof>& proofs,
                        const std::vector<std::vector<Fr>>& values, unsigned log2n, bool extended, bool bit_reversed,
                        bool checked, bool check_subgroup, std::vector<bool>* each = nullptr);
  bool shplonk_verified(std::vector<commit>& commits, const std::vector<Fr>& points,
                        const std::vector<shplonk_set>& sets, const Fr& gamma,
                        const std::vector<std::vector<Fr>>& values, const Fr& z, shplonk_proof& proof, bool checked,
                        bool check_subgroup);
  std::vector<Fr> recovered(const std::vector<uint32_t>& cell_index, const std::vector<std::vector<Fr>>& values,
                            unsigned log2n, bool bit_reversed, std::vector<proof>* proofs);
  bool batch_verified(std::vector<commit>& commits, const std::vector<batch_opening>& groups,
                      const std::vector<Fr>& gammas, const std::vector<std::vector<Fr>>& values,
                      std::vector<proof>& proofs, bool checked, bool check_subgroup);

 public:
  /** random tau (std::random_device), [tau^i]G1 and [tau^i]G2 for
   *  i < num_coeff, on the GPU  @throws std::invalid_argument if num_coeff < 2 */
  trusted_setup(int num_coeff);
  /** Extension: deterministic setup from a given tau (tests, benchmarks). */
  trusted_setup(int num_coeff, const Fr& tau);
  /** load a setup written by export_setup (trusted_setup.cpp:76-121)
   *  @throws std::runtime_error for an inaccessible file or a bad G1 record,
   *          std::logic_error for a bad G2 record (as the reference does) */
  trusted_setup(const std::string& filename);
  /** Extension: a setup from packed compressed points, as published setups
   *  come: g1 holds 48-byte and g2 96-byte KZGX_ENC_ZCASH records (BLS12-381).
   *  The counts are independent (a cell verifier's setup has 64 G1 and 65 G2
   *  points).  Decompressed and checked on the GPU (on the curve, and with
   *  check_subgroup in the prime-order subgroup), then installed as a loaded
   *  file's points are; size() is the G1 count.
   *  @throws std::invalid_argument on BN254, for an empty array or a size that
   *          is not a multiple of the record length; std::runtime_error for a
   *          bad or infinite G1 record, std::logic_error for a G2 one (as the
   *          file constructor does) */
  static trusted_setup from_compressed(const std::vector<uint8_t>& g1, const std::vector<uint8_t>& g2,
                                       bool check_subgroup = true);
  ~trusted_setup();
  trusted_setup(const trusted_setup&) = delete;
  trusted_setup& operator=(const trusted_setup&) = delete;
  trusted_setup(trusted_setup&& o) noexcept;
  trusted_setup& operator=(trusted_setup&& o) noexcept;

  size_t size() const { return n; }

  /** C = [P(s)]1  @throws std::invalid_argument if deg(P) + 1 >= size() */
  commit create_commit(const kzg::poly& poly);
  bool verify_commit(kzg::commit& commit, const kzg::poly& poly);
  /** @throws std::invalid_argument on chunk_size / alignment violations */
  proof create_proof(const kzg::poly& poly, int byte_offset, int byte_length, int chunk_size);
  /** @throws std::invalid_argument if chunk_length < 1 */
  proof create_proof(const kzg::poly& poly, int chunk_offset, int chunk_length);
  /** e(proof, [Z(s)]2) == e(C - [I(s)]1, [1]2), all on the GPU
   *  (trusted_setup.cpp:230-254)
   *  @throws std::invalid_argument if expected_data is empty; false if it
   *          holds >= size() points */
  bool verify_proof(commit& commit, proof& proof, blob& expected_data);
  /** writes the reference file layout (trusted_setup.cpp:256-287):
   *  u64 n, n x (u32 len, G1 octet), n x (u32 len, G2 octet); prints
   *  "failed to export" and returns if the file cannot be opened */
  void export_setup(const std::string& filename = "kzg_public");

  /** Extensions: batched commits / single-point openings in one GPU pass. */
  std::vector<commit> create_commits(const std::vector<kzg::poly>& polys);
  std::vector<proof> create_proofs(const kzg::poly& poly, const std::vector<long>& points);
  /** Extension: commitments of polynomials given by their values on the
   *  size-2^k domain (all vectors of that size), one GPU pass: inverse NTT,
   *  then the batched MSM (kzgx_commit_evals_batch).  Equal to
   *  create_commits of poly::from_evaluations of each vector.
   *  @throws std::invalid_argument if the size is not a power of two, exceeds
   *          the curve's domain, differs between vectors, or 2^k >= size() */
  std::vector<commit> create_commits_from_evaluations(const std::vector<std::vector<Fr>>& evals,
                                                      bool bit_reversed = false);
  /** Extension: single-point openings at `points` (any scalars, domain points
   *  included) of the polynomial given by `evals` (kzgx_prove_evals_batch).
   *  @throws std::invalid_argument as create_commits_from_evaluations */
  std::vector<proof> create_proofs_from_evaluations(const std::vector<Fr>& evals, const std::vector<Fr>& points,
                                                    bool bit_reversed = false);
  /** Extension: the 2^log2n single-point openings of p at every point of the
   *  size-2^log2n domain in one GPU pass of Theta(n log n) group operations
   *  (kzgx_prove_all_batch): element i opens at w^i, w = domain_root(log2n), or
   *  with bit_reversed element (bit reversal of i).  Each equals
   *  create_proofs_from_evaluations at that point.
   *  @throws std::invalid_argument if deg + 1 > 2^log2n, the twice larger
   *          domain exceeds the curve's (BN254: log2n > 1), or 2^log2n >= size() */
  std::vector<proof> create_all_proofs(const poly& p, unsigned log2n, bool bit_reversed = false);
  /** Extension: the same for the polynomial given by its values on the domain
   *  (bit-reversed on both sides with bit_reversed).
   *  @throws std::invalid_argument as create_commits_from_evaluations and create_all_proofs */
  std::vector<proof> create_all_proofs_from_evaluations(const std::vector<Fr>& evals, bool bit_reversed = false);
  /** Extension: one opening per coset (cell) of 2^log2l points in one GPU pass
   *  (kzgx_prove_cosets_batch): the cosets of the size-2^log2n domain, or with
   *  `extended` of the twice larger one (2^(log2n - log2l + 1) cells, the
   *  data-availability layout).  Element i opens the points w^(i + R j),
   *  j < 2^log2l, R the number of cosets, w = domain_root(log2 of R 2^log2l);
   *  with bit_reversed element (bit reversal of i).  kzgx_coset_points lists a
   *  cell's points; each proof equals the multi-point opening at them.
   *  @throws std::invalid_argument as create_all_proofs, for log2l > log2n, or
   *          if the size-2^(log2n - log2l + 1) or the opened domain exceeds the
   *          curve's */
  std::vector<proof> create_coset_proofs(const poly& p, unsigned log2n, unsigned log2l, bool extended = false,
                                         bool bit_reversed = false);
  /** Extension: the same for the polynomial given by its values on the
   *  size-n domain (bit-reversed over n with bit_reversed).
   *  @throws std::invalid_argument as create_commits_from_evaluations and create_coset_proofs */
  std::vector<proof> create_coset_proofs_from_evaluations(const std::vector<Fr>& evals, unsigned log2l,
                                                          bool extended = false, bool bit_reversed = false);
  /** Extension: many single-point verify_proof calls in one GPU pass;
   *  result k == verify_proof(commits[k], proofs[k], blob {points[k]}). */
  std::vector<bool> verify_proofs(std::vector<commit>& commits, std::vector<proof>& proofs,
                                  const std::vector<std::pair<Fr, Fr>>& points);
  /** Extension: one pairing check for all openings (kzgx_verify_aggregate
   *  with library-drawn 128-bit challenges); true iff every (commits[k],
   *  proofs[k], points[k]) verifies (false-accept probability <= 2^-128).
   *  On false, verify_proofs() says which.  An empty batch is true.
   *  @throws std::invalid_argument on mismatched sizes */
  bool verify_proofs_aggregated(std::vector<commit>& commits, std::vector<proof>& proofs,
                                const std::vector<std::pair<Fr, Fr>>& points);
  /** Extension: the same behind a validation of every commit and proof
   *  (kzgx_verify_aggregate_checked): canonical and on the curve, and with
   *  check_subgroup in the prime-order subgroup; false as soon as one point
   *  fails, whatever the pairing equation says. */
  bool verify_proofs_aggregated(std::vector<commit>& commits, std::vector<proof>& proofs,
                                const std::vector<std::pair<Fr, Fr>>& points, bool check_subgroup);
  /** Extension: one pairing check for many coset openings (cells) of several
   *  commitments (kzgx_verify_cells_aggregate with library-drawn 128-bit
   *  challenges).  Cell k opens commits[commit_index[k]] on coset cell_index[k]
   *  of create_coset_proofs' layout for (log2n, extended), with proofs[k] and
   *  the 2^log2l values values[k] in the coset's point order; log2l is taken
   *  from the values' length.  With bit_reversed cell_index[k] is the element
   *  number of create_coset_proofs(..., bit_reversed = true) and values[k] the
   *  matching chunk of the bit-reversed evaluation array, as they come.  Each
   *  commitment is passed once.  True iff every cell verifies (false-accept
   *  probability <= 2^-128); on false, verify_coset_proofs_each says which.
   *  An empty batch is true.  Needs
   *  only 2^log2l G1 and 2^log2l + 1 G2 setup points, whatever log2n.
   *  @throws std::invalid_argument on mismatched sizes, values whose length is
   *          not one power of two shared by all cells, an index out of range,
   *          log2l > log2n, or a domain beyond the curve's */
  bool verify_coset_proofs(std::vector<commit>& commits, const std::vector<uint32_t>& commit_index,
                           const std::vector<uint32_t>& cell_index, std::vector<proof>& proofs,
                           const std::vector<std::vector<Fr>>& values, unsigned log2n, bool extended = false,
                           bool bit_reversed = false);
  /** Extension: the same behind a validation of every commit and proof
   *  (kzgx_verify_cells_aggregate_checked): canonical and on the curve, and
   *  with check_subgroup in the prime-order subgroup; false as soon as one
   *  point fails, whatever the pairing equation says. */
  bool verify_coset_proofs(std::vector<commit>& commits, const std::vector<uint32_t>& commit_index,
                           const std::vector<uint32_t>& cell_index, std::vector<proof>& proofs,
                           const std::vector<std::vector<Fr>>& values, unsigned log2n, bool extended,
                           bool bit_reversed, bool check_subgroup);
  /** Extension: the same batch, one verdict per cell (kzgx_verify_cells_each):
   *  element k is what verify_proof answers for cell k over the points
   *  kzgx_coset_points lists -- exact and deterministic, no challenges, so
   *  errors that would cancel in the aggregate are each reported.  One batched
   *  GPU pipeline for the whole list, not a call per cell.  An empty batch
   *  gives an empty vector.  Setup points and exceptions as
   *  verify_coset_proofs. */
  std::vector<bool> verify_coset_proofs_each(std::vector<commit>& commits, const std::vector<uint32_t>& commit_index,
                                             const std::vector<uint32_t>& cell_index, std::vector<proof>& proofs,
                                             const std::vector<std::vector<Fr>>& values, unsigned log2n,
                                             bool extended = false, bool bit_reversed = false);
  /** Extension: the same behind a validation of every commit and proof
   *  (kzgx_verify_cells_each_checked): a cell whose proof or commitment is not
   *  canonical, not on the curve or, with check_subgroup, outside the
   *  prime-order subgroup is false; the other cells keep their verdicts. */
  std::vector<bool> verify_coset_proofs_each(std::vector<commit>& commits, const std::vector<uint32_t>& commit_index,
                                             const std::vector<uint32_t>& cell_index, std::vector<proof>& proofs,
                                             const std::vector<std::vector<Fr>>& values, unsigned log2n, bool extended,
                                             bool bit_reversed, bool check_subgroup);
  /** Extension: the checked form on compressed commitments and proofs as they
   *  travel (kzgx_verify_cells_aggregate_bytes): `commits` and `proofs` hold
   *  whole records of `encoding` back to back, decompressed and checked in one
   *  GPU launch in front of the aggregate; a record that does not decode makes
   *  the answer false.
   *  @throws std::invalid_argument as above, for an encoding the curve does not
   *          offer, or a size that is not a multiple of the record length */
  bool verify_coset_proofs(const std::vector<uint8_t>& commits, const std::vector<uint32_t>& commit_index,
                           const std::vector<uint32_t>& cell_index, const std::vector<uint8_t>& proofs,
                           const std::vector<std::vector<Fr>>& values, unsigned log2n, bool extended,
                           bool bit_reversed, int encoding, bool check_subgroup = true);
  /** Extension: rebuild one erasure-coded blob from at least half of its cells
   *  (kzgx_recover_cells): the cells are those of create_coset_proofs(p, log2n,
   *  log2l, extended = true, bit_reversed), cell_index[k] the element number and
   *  values[k] its 2^log2l values in the coset's point order (log2l is taken
   *  from the values' length).  Returns all 2^(log2n + 1) values in
   *  kzgx_prove_cosets_batch's y layout for the same order: cell i is elements
   *  i 2^log2l .. (i + 1) 2^log2l - 1.  Needs no setup points.
   *  @throws std::invalid_argument on mismatched sizes, values whose length is
   *          not one power of two shared by all cells, an index out of range, a
   *          cell given twice, fewer than half the cells, log2l > log2n, more
   *          than 2^KZGX_RECOVER_MAX_LOG2_CELLS cells, or a domain beyond the
   *          curve's
   *  @throws std::domain_error if no polynomial of fewer than 2^log2n
   *          coefficients takes every given value (only detectable with more
   *          than half the cells) */
  std::vector<Fr> recover_cells(const std::vector<uint32_t>& cell_index, const std::vector<std::vector<Fr>>& values,
                                unsigned log2n, bool bit_reversed = false);
  /** Extension: the same with every cell's proof recomputed
   *  (kzgx_recover_cells_and_proofs): the values and create_coset_proofs'
   *  output for the recovered polynomial.
   *  @throws as recover_cells and create_coset_proofs */
  std::pair<std::vector<Fr>, std::vector<proof>> recover_cells_and_proofs(
      const std::vector<uint32_t>& cell_index, const std::vector<std::vector<Fr>>& values, unsigned log2n,
      bool bit_reversed = false);
  /** Extension: blob proofs (kzgx_prove_blobs_batch; BLS12-381 only).  `blobs`
   *  holds whole blobs back to back, 2^log2n elements of 32 big-endian bytes
   *  each, the values of a polynomial on the size-2^log2n domain (bit-reversed
   *  order by default, as data-availability blobs come).  Returns the
   *  commitments and the proofs as 48-byte KZGX_ENC_ZCASH records, back to
   *  back: proof b opens blob b at its Fiat-Shamir challenge
   *  z = H(blob || commitment) (kzg_gpu.h "blob proofs" has the layout).  One
   *  batched GPU pipeline for all blobs.
   *  @throws std::invalid_argument on BN254, a size that is not a whole number
   *          of blobs, an element >= r, more than 65535 blobs, a domain beyond
   *          the curve's or the setup */
  std::pair<std::vector<uint8_t>, std::vector<uint8_t>> create_blob_proofs(const std::vector<uint8_t>& blobs,
                                                                           unsigned log2n, bool bit_reversed = true);
  /** Extension: one answer for all blobs (kzgx_verify_blobs_batch): records
   *  decompressed and checked (with check_subgroup in the prime-order
   *  subgroup), challenges hashed and values evaluated on the GPU, then ONE
   *  pairing check under library-drawn 128-bit challenges.  False when a record
   *  does not decode or an element is >= r.  No blobs: true.
   *  @throws std::invalid_argument on BN254, mismatched sizes, too many blobs
   *          (KZGX_MSM_POINTS_MAX / 2 - 1) or a domain beyond the curve's */
  bool verify_blob_proofs(const std::vector<uint8_t>& blobs, const std::vector<uint8_t>& commits,
                          const std::vector<uint8_t>& proofs, unsigned log2n, bool bit_reversed = true,
                          bool check_subgroup = true);
  /** Extension: the same batch, one exact verdict per blob
   *  (kzgx_verify_blobs_each): a blob whose own record or element is invalid
   *  is false and no other blob is affected.
   *  @throws as verify_blob_proofs */
  std::vector<bool> verify_blob_proofs_each(const std::vector<uint8_t>& blobs, const std::vector<uint8_t>& commits,
                                            const std::vector<uint8_t>& proofs, unsigned log2n,
                                            bool bit_reversed = true, bool check_subgroup = true);
  /** Extension: every installed G1 and G2 point is canonical, on its curve
   *  and (subgroup) in the prime-order subgroup (kzgx_srs_check, on the
   *  device).  trusted_setup(filename) tests on-curve only: call this after
   *  loading a file you did not write.  It tests each point on its own:
   *  whether the points are consecutive powers of one tau is
   *  verify_structure()'s question. */
  bool check_setup(bool subgroup = true);
  /** Extension: one powers-of-tau contribution (kzgx_srs_update): point i of
   *  both halves is multiplied by s^i on the GPU, so a setup for tau becomes
   *  one for tau s, and every table and cached setup follows.  Returns the
   *  witness [s]G2 that verify_contribution needs.  No transcript format, no
   *  chain verifier, no hashing of s: s is the caller's to draw and forget.
   *  @throws std::invalid_argument if s is zero */
  G2 contribute(const Fr& s);
  /** Extension: the installed points are consecutive powers of one tau in
   *  both groups (kzgx_srs_verify_structure: two MSMs per group under random
   *  challenges and two pairing equations), and with `generators` they start
   *  at the curve's generators, as every setup this library generates does.
   *  Meaningful only for subgroup members: call check_setup() first.  A wrong
   *  setup passes with probability about size() / 2^128. */
  bool verify_structure(bool generators = true);
  /** Extension: e(new_tau, G2) == e(prev_tau, witness), witness and new_tau
   *  finite (kzgx_srs_verify_update): new_tau = g1_points()[1] after a
   *  contribution whose predecessor's was prev_tau. */
  static bool verify_contribution(const G1& prev_tau, const G1& new_tau, const G2& witness);
  /** Extension: sum scalars[k] * points[k] on the GPU (kzgx_msm_g1_points).
   *  KZG commitments are additively homomorphic: the combination of
   *  commitments is the commitment of the combined polynomials.
   *  @throws std::invalid_argument on mismatched sizes */
  G1 linear_combination(const std::vector<G1>& points, const std::vector<Fr>& scalars);
  /** Extension: batch openings (kzgx_prove_multi_batch with
   *  KZGX_MULTI_WEIGHT_POWERS): ONE proof per group instead of one per
   *  (polynomial, point) pair.  Proof g opens F_g = sum_j gammas[g]^j
   *  polys[groups[g].polys[j]] at groups[g].point: one fold over the
   *  coefficients and one MSM per group, all groups in one batched pipeline.
   *  values_out (optional) receives, group by group in the order of `polys`
   *  lists, every polynomial's own value at its group's point -- what the
   *  verifier is told.  The caller derives the gammas (nothing is hashed here).
   *  @throws std::invalid_argument on mismatched sizes, an index beyond
   *          `polys`, or a degree beyond the setup */
  std::vector<proof> create_batch_proofs(const std::vector<kzg::poly>& polys, const std::vector<batch_opening>& groups,
                                         const std::vector<Fr>& gammas,
                                         std::vector<std::vector<Fr>>* values_out = nullptr);
  /** Extension: the verifier's side (kzgx_verify_multi_batch): `values[g][j]`
   *  is the claimed value of commits[groups[g].polys[j]] at groups[g].point.
   *  Two variable-base MSMs and ONE pairing check for the whole batch, under
   *  library-drawn 128-bit challenges across the groups.  The second form runs
   *  the G1 check of every commitment and proof first (check_subgroup: also
   *  prime-order membership) and is false when one fails.  No groups: true.
   *  @throws std::invalid_argument on mismatched sizes or an index beyond
   *          `commits` */
  bool verify_batch_proofs(std::vector<commit>& commits, const std::vector<batch_opening>& groups,
                           const std::vector<Fr>& gammas, const std::vector<std::vector<Fr>>& values,
                           std::vector<proof>& proofs);
  bool verify_batch_proofs(std::vector<commit>& commits, const std::vector<batch_opening>& groups,
                           const std::vector<Fr>& gammas, const std::vector<std::vector<Fr>>& values,
                           std::vector<proof>& proofs, bool check_subgroup);
  /** Extension: Shplonk openings (kzgx_shplonk_commit, kzgx_shplonk_open with
   *  KZGX_SHPLONK_WEIGHT_POWERS): different polynomials opened at different
   *  point sets under ONE proof of two G1 points.  Claim k, counted over the
   *  sets in order, has the weight gamma^k.  `challenge` is called once, with
   *  W, between the two steps and returns z: it must hash W (and what gamma
   *  hashed), nothing is hashed here.  values_out (optional) receives, set by
   *  set, every named polynomial's values at the set's points: polynomial j
   *  of the set's list at [j * points.size(), (j + 1) * points.size()).
   *  @throws std::invalid_argument on an index beyond `polys` or `points`, an
   *          index twice in one set, an empty point list or a degree beyond
   *          the setup; std::domain_error on equal point values in one set */
  shplonk_proof create_shplonk_proof(const std::vector<kzg::poly>& polys, const std::vector<Fr>& points,
                                     const std::vector<shplonk_set>& sets, const Fr& gamma,
                                     const std::function<Fr(const proof&)>& challenge,
                                     std::vector<std::vector<Fr>>* values_out = nullptr);
  /** Extension: the verifier's side (kzgx_shplonk_verify): `values` as
   *  values_out above, z the challenge.  Two variable-base MSMs and ONE
   *  pairing check.  The second form runs the G1 check of every commitment and
   *  of both proof points first (check_subgroup: also prime-order membership)
   *  and is false when one fails.
   *  @throws std::invalid_argument on mismatched sizes or a malformed table,
   *          as above */
  bool verify_shplonk_proof(std::vector<commit>& commits, const std::vector<Fr>& points,
                            const std::vector<shplonk_set>& sets, const Fr& gamma,
                            const std::vector<std::vector<Fr>>& values, const Fr& z, shplonk_proof& proof);
  bool verify_shplonk_proof(std::vector<commit>& commits, const std::vector<Fr>& points,
                            const std::vector<shplonk_set>& sets, const Fr& gamma,
                            const std::vector<std::vector<Fr>>& values, const Fr& z, shplonk_proof& proof,
                            bool check_subgroup);
  /** copy of the G1 / G2 SRS points */
  std::vector<G1> g1_points() const;
  std::vector<G2> g2_points() const;
  /** Extension: precompute the fixed-base table of odd multiples for the
   *  first `points` SRS points (0 = all) with `window_bits`-bit windows
   *  (kzgx_set_fixed_base).  Entries are 64 B (BN254) / 112 B (BLS12-381);
   *  over 4097 points BN254 c = 17 (15 windows, the bench's table) takes
   *  257.8 GB of HBM, c = 16 137.5 GB, c = 12 11.8 GB, and BLS12-381 c = 16
   *  240.6 GB.  Commits and proofs over that prefix then run as plain table
   *  sums.  window_bits = 0 drops the table.  Without it, batches run on
   *  the default table below.  These byte counts are the footprint: for
   *  1024 .. 16384 points the library splits it between a block table of
   *  cross-point subset sums, which serves batches of >= 64 commits or
   *  proofs, and a narrower window table for single calls (BN254 c = 17:
   *  176.1 + 73.0 GB; kzgx_set_fixed_joint in kzg_gpu.h turns that off). */
  void precompute(int window_bits = 16, size_t points = 0);
  /** Extension: the default table (kzgx_set_default_table), built with
   *  every setup: odd multiples of the first 4097 SRS points at the widest
   *  window c <= 12 that fits 4.5% of the HBM (window_bits = -1, the default:
   *  BN254 c = 12, 11.8 GB; BLS12-381 c = 11, 9.7 GB).  Single create_commit /
   *  create_proof calls of degree <= 4096 take its one-launch path, batches
   *  its batched kernel.  The reference's create_commit allocates nothing
   *  beyond the SRS (src/trusted_setup.cpp:137-142): default_table(0)
   *  restores that, and every MSM then runs the table-less Pippenger. */
  void default_table(int window_bits, size_t points = 4097);
  /** Extension: the widest window whose table over `points` SRS points
   *  (0 = all) fits `budget_bytes` and the free HBM; returns the window
   *  built (0: none fits, Pippenger stays).  DESIGN.md section 3 holds the
   *  measured throughput at each table size. */
  int precompute_budget(size_t budget_bytes, size_t points = 0);
};

}  // namespace kzg

#endif
