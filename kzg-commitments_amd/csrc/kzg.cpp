// C++ facade: the reference's kzg:: API (/root/reference/src/kzg.h) over the
// C ABI of libkzgx.so.  Host code here only validates arguments, converts
// byte formats and marshals; every field / group computation is a GPU call.
#include "../../include/kzg.h"

#include <algorithm>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <mutex>
#include <random>

#include "curve_consts.h"

namespace kzg {

int CURVE_ORDER_BYTES;

namespace {

int g_curve = KZGX_CURVE_BN254;
int g_device = 0;  // kzg::set_device
std::mutex g_mu;
// default contexts for the setup-independent poly ops, one per (curve,
// device), created on first use and kept until process exit: init() and
// set_device() only switch which one default_ctx() hands out, so a pointer
// another thread obtained earlier stays valid
std::map<std::pair<int, int>, kzgx_ctx*> g_ctxs;

void check(int rc, const char* where) {
  if (rc == KZGX_OK) return;
  std::string msg = std::string(where) + ": " + kzgx_strerror(rc);
  if (rc == KZGX_ERR_ARG || rc == KZGX_ERR_DEGREE) throw std::invalid_argument(msg);
  if (rc == KZGX_ERR_DIV_ZERO) throw std::domain_error(msg);
  throw std::runtime_error(msg);
}

kzgx_ctx* default_ctx() {
  std::lock_guard<std::mutex> lk(g_mu);
  kzgx_ctx*& c = g_ctxs[{g_curve, g_device}];
  if (!c) check(kzgx_create(&c, g_curve, g_device), "kzgx_create");
  return c;
}

// r as 64-bit limbs for the selected curve
std::array<uint64_t, 4> order() {
  const uint32_t* w = g_curve == KZGX_CURVE_BN254 ? kzgx::BN254Fr::P : kzgx::BLS12381Fr::P;
  std::array<uint64_t, 4> r{};
  for (int i = 0; i < 4; i++) r[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
  return r;
}

bool geq(const std::array<uint64_t, 4>& a, const std::array<uint64_t, 4>& b) {
  for (int i = 3; i >= 0; i--)
    if (a[i] != b[i]) return a[i] > b[i];
  return true;
}

void sub_in(std::array<uint64_t, 4>& a, const std::array<uint64_t, 4>& b) {
  unsigned __int128 br = 0;
  for (int i = 0; i < 4; i++) {
    unsigned __int128 t = (unsigned __int128)a[i] - b[i] - br;
    a[i] = (uint64_t)t;
    br = (t >> 64) & 1;
  }
}

// x mod r for a 256-bit x (x < 2^256 < 8 r on both curves)
void reduce(std::array<uint64_t, 4>& a) {
  const auto r = order();
  while (geq(a, r)) sub_in(a, r);
}

int base_limbs() { return kzgx_base_limbs(g_curve); }
size_t mod_bytes() { return g_curve == KZGX_CURVE_BN254 ? 32 : 48; }

std::vector<uint64_t> flat(const std::vector<Fr>& P) {
  std::vector<uint64_t> out(4 * P.size());
  for (size_t i = 0; i < P.size(); i++) std::memcpy(&out[4 * i], P[i].v.data(), 32);
  return out;
}

G1 to_g1(const uint64_t* xy, int inf) {
  G1 g;
  const int nl = base_limbs();
  g.inf = inf != 0;
  if (!g.inf)
    for (int i = 0; i < nl; i++) {
      g.x[i] = xy[i];
      g.y[i] = xy[nl + i];
    }
  return g;
}

// ECP_toOctet(..., false): 0x04 || X || Y big-endian (util.cpp:78-96).
// Infinity: miracl's ECP_inf is (0, 1), so the octet is 04 || 0 || 1.
std::vector<uint8_t> ecp_serialize(const G1& g) {
  const size_t mb = mod_bytes();
  const int nl = base_limbs();
  std::vector<uint8_t> oct(1 + 2 * mb, 0);
  oct[0] = 0x04;
  std::array<uint64_t, 6> x = g.x, y = g.y;
  if (g.inf) {
    x.fill(0);
    y.fill(0);
    y[0] = 1;
  }
  for (size_t k = 0; k < mb; k++) {
    oct[1 + mb - 1 - k] = (uint8_t)(x[k / 8] >> (8 * (k % 8)));
    oct[1 + 2 * mb - 1 - k] = (uint8_t)(y[k / 8] >> (8 * (k % 8)));
  }
  (void)nl;
  std::vector<uint8_t> out(4);
  uint32_t len = (uint32_t)oct.size();
  std::memcpy(out.data(), &len, 4);
  out.insert(out.end(), oct.begin(), oct.end());
  return out;
}

// ECP2_toOctet(..., false): 0x04 || x || y, each Fp2 as imag || real,
// MODBYTES big-endian each (miracl-core's current FP2_toBytes order; recalled,
// version-dependent).  Infinity: ECP2_inf = (0, 1).
void put_be(uint8_t* dst, const uint64_t* limbs, size_t mb) {
  for (size_t k = 0; k < mb; k++) dst[mb - 1 - k] = (uint8_t)(limbs[k / 8] >> (8 * (k % 8)));
}
void get_be(const uint8_t* src, uint64_t* limbs, size_t mb) {
  for (size_t k = 0; k < mb; k++) limbs[k / 8] |= (uint64_t)src[mb - 1 - k] << (8 * (k % 8));
}

std::vector<uint8_t> ecp2_octet(const G2& g) {
  const size_t mb = mod_bytes();
  std::vector<uint8_t> oct(1 + 4 * mb, 0);
  oct[0] = 0x04;
  std::array<uint64_t, 6> x0 = g.x0, x1 = g.x1, y0 = g.y0, y1 = g.y1;
  if (g.inf) {
    x0.fill(0);
    x1.fill(0);
    y0.fill(0);
    y1.fill(0);
    y0[0] = 1;
  }
  put_be(&oct[1], x1.data(), mb);
  put_be(&oct[1 + mb], x0.data(), mb);
  put_be(&oct[1 + 2 * mb], y1.data(), mb);
  put_be(&oct[1 + 3 * mb], y0.data(), mb);
  return oct;
}

// G2 canonical words (x.re, x.im, y.re, y.im; base_limbs() each) <-> G2
G2 to_g2(const uint64_t* w, bool inf) {
  G2 g;
  const int nl = base_limbs();
  g.inf = inf;
  if (!inf)
    for (int i = 0; i < nl; i++) {
      g.x0[i] = w[i];
      g.x1[i] = w[nl + i];
      g.y0[i] = w[2 * nl + i];
      g.y1[i] = w[3 * nl + i];
    }
  return g;
}

// deserialize_ECP (util.cpp:98-115): anything that is not a valid on-curve
// octet decodes to infinity.  The on-curve test runs on the GPU (g1_sum of
// the single point is the identity iff the point is valid).
// the octet's coordinates (not yet validated); false for a malformed octet
bool ecp_parse(const std::vector<uint8_t>& bytes, G1& g) {
  if (bytes.size() < 4) return false;
  uint32_t len;
  std::memcpy(&len, bytes.data(), 4);
  const size_t mb = mod_bytes();
  if (len != 1 + 2 * mb || bytes.size() < 4 + len || bytes[4] != 0x04) return false;
  g = G1();
  g.inf = false;
  for (size_t k = 0; k < mb; k++) {
    g.x[k / 8] |= (uint64_t)bytes[4 + 1 + mb - 1 - k] << (8 * (k % 8));
    g.y[k / 8] |= (uint64_t)bytes[4 + 1 + 2 * mb - 1 - k] << (8 * (k % 8));
  }
  return true;
}

G1 ecp_deserialize(const std::vector<uint8_t>& bytes) {
  G1 inf;
  G1 g;
  if (!ecp_parse(bytes, g)) return inf;
  // validity: the GPU sums [P] alone and returns it canonically only if P is
  // a proper curve point (coordinates < p and y^2 = x^3 + b)
  const int nl = base_limbs();
  std::vector<uint64_t> xy(2 * nl);
  for (int i = 0; i < nl; i++) {
    xy[i] = g.x[i];
    xy[nl + i] = g.y[i];
  }
  int ok = 0;
  check(kzgx_g1_validate(default_ctx(), xy.data(), &ok), "kzgx_g1_validate");
  return ok ? g : inf;
}

// ecp_deserialize of every entry with ONE kzgx_g1_check_batch: the host only
// parses octets.  Malformed octets and all-zero coordinates (not an octet
// point: kzgx_g1_validate rejects them) go to the device as infinite entries
// and are marked invalid here.
std::vector<G1> ecp_deserialize_batch(const std::vector<std::vector<uint8_t>>& bytes, bool check_subgroup,
                                      std::vector<bool>* valid) {
  const size_t m = bytes.size();
  const int nl = base_limbs();
  std::vector<G1> res(m);
  std::vector<uint64_t> xy(2 * nl * m + 1, 0);
  std::vector<int> ok(m + 1, 0);
  std::vector<bool> parsed(m, false);
  for (size_t k = 0; k < m; k++) {
    G1 g;
    if (!ecp_parse(bytes[k], g)) continue;
    uint64_t any = 0;
    for (int i = 0; i < nl; i++) {
      xy[2 * nl * k + i] = g.x[i];
      xy[2 * nl * k + nl + i] = g.y[i];
      any |= g.x[i] | g.y[i];
    }
    parsed[k] = any != 0;
    res[k] = g;
  }
  if (m) check(kzgx_g1_check_batch(default_ctx(), xy.data(), nullptr, m, check_subgroup ? 1 : 0, ok.data()),
               "kzgx_g1_check_batch");
  if (valid) valid->assign(m, false);
  for (size_t k = 0; k < m; k++) {
    const bool good = parsed[k] && ok[k] != 0;
    if (!good) res[k] = G1();
    if (valid) (*valid)[k] = good;
  }
  return res;
}

// the record length of (the selected curve, G1 / G2, encoding), or invalid_argument
size_t record_bytes(int group, int encoding) {
  const size_t rb = kzgx_point_bytes(g_curve, group, encoding);
  if (rb == 0) throw std::invalid_argument("compressed points: the curve does not offer this encoding");
  return rb;
}

std::vector<uint8_t> g1_compressed(const G1& g, int encoding) {
  std::vector<uint8_t> out(record_bytes(1, encoding));
  const int nl = base_limbs();
  std::vector<uint64_t> xy(2 * nl, 0);
  for (int i = 0; i < nl; i++) {
    xy[i] = g.x[i];
    xy[nl + i] = g.y[i];
  }
  const int inf = g.inf;
  check(kzgx_g1_compress_batch(default_ctx(), xy.data(), &inf, 1, encoding, out.data()), "kzgx_g1_compress_batch");
  return out;
}

// every record of `packed` with ONE kzgx_g1_decompress_batch: the host splits nothing and computes nothing
std::vector<G1> g1_decompress_packed(const std::vector<uint8_t>& packed, int encoding, bool check_subgroup,
                                     std::vector<bool>* valid) {
  const size_t rb = record_bytes(1, encoding);
  if (packed.size() % rb) throw std::invalid_argument("compressed points: not a whole number of records");
  const size_t m = packed.size() / rb;
  const int nl = base_limbs();
  std::vector<uint64_t> xy(2 * nl * m + 1, 0);
  std::vector<int> inf(m + 1, 0), ok(m + 1, 0);
  check(kzgx_g1_decompress_batch(default_ctx(), packed.data(), m, encoding, check_subgroup ? 1 : 0, xy.data(),
                                 inf.data(), ok.data()),
        "kzgx_g1_decompress_batch");
  std::vector<G1> res(m);
  if (valid) valid->assign(m, false);
  for (size_t k = 0; k < m; k++) {
    if (valid) (*valid)[k] = ok[k] != 0;
    if (inf[k]) continue;
    res[k].inf = false;
    for (int i = 0; i < nl; i++) {
      res[k].x[i] = xy[2 * nl * k + i];
      res[k].y[i] = xy[2 * nl * k + nl + i];
    }
  }
  return res;
}

}  // namespace

// ---- Fr ---------------------------------------------------------------------
Fr::Fr(long x) {
  unsigned long m = x < 0 ? (unsigned long)(-(x + 1)) + 1ul : (unsigned long)x;
  v = {m, 0, 0, 0};
  reduce(v);
  if (x < 0 && !is_zero()) {
    auto r = order();
    sub_in(r, v);
    v = r;
  }
}

Fr Fr::from_le_bytes(const uint8_t* bytes, size_t n) {
  Fr f;
  // NTL ZZFromBytes then conv<ZZ_p>: reduce mod r; inputs here are <= 32 bytes
  std::array<uint64_t, 4> a{};
  for (size_t k = 0; k < n && k < 32; k++) a[k / 8] |= (uint64_t)bytes[k] << (8 * (k % 8));
  for (size_t k = 32; k < n; k++)
    if (bytes[k]) throw std::invalid_argument("Fr::from_le_bytes: value wider than 256 bits");
  reduce(a);
  f.v = a;
  return f;
}

std::vector<uint8_t> Fr::to_le_bytes() const {
  std::vector<uint8_t> out;
  for (int k = 0; k < 32; k++) out.push_back((uint8_t)(v[k / 8] >> (8 * (k % 8))));
  while (!out.empty() && out.back() == 0) out.pop_back();  // NumBytes
  return out;
}

// ---- init -------------------------------------------------------------------
void init() { init(KZGX_CURVE_BN254); }

void init(int curve) {
  if (curve != KZGX_CURVE_BN254 && curve != KZGX_CURVE_BLS12381) throw std::invalid_argument("unknown curve");
  int dev;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    g_curve = curve;
    CURVE_ORDER_BYTES = 32;  // NumBytes(r) on both curves (trusted_setup.cpp:18)
    dev = g_device;
  }
  // the reference's init sets up its curve state before any other call
  // (src/kzg.h:33-38); here that is the device: HIP, every code object and
  // the generator tables, so no later call pays them.  Without a gfx950
  // device init still succeeds and the first GPU call throws.
  const int rc = kzgx_init_device(curve, dev);
  if (rc == KZGX_ERR_NO_DEVICE) return;
  check(rc, "kzgx_init_device");
  (void)default_ctx();
}

int curve() { return g_curve; }

void set_device(int device) {
  if (device < 0) throw std::invalid_argument("negative device ordinal");
  std::lock_guard<std::mutex> lk(g_mu);
  g_device = device;
}

int device() {
  std::lock_guard<std::mutex> lk(g_mu);
  return g_device;
}

// ---- blob -------------------------------------------------------------------
blob blob::from_string(std::string s) { return from_string(s, 0); }

blob blob::from_string(std::string s, int offset) {
  std::vector<std::pair<Fr, Fr>> d;
  d.reserve(s.size());
  for (size_t i = 0; i < s.size(); i++) d.push_back({Fr((long)i + offset), Fr((long)(signed char)s[i])});
  return blob(d);
}

blob blob::from_bytes(const uint8_t* bytes, int byte_offset, int byte_length, int chunk_size) {
  if (chunk_size > MAX_CHUNK_BYTES) throw std::invalid_argument("chunk_size must be at most MAX_CHUNK_BYTES.");
  if (chunk_size < 1) throw std::invalid_argument("chunk_size must be at least 1.");  // reference: UB
  if (byte_offset % chunk_size != 0) throw std::invalid_argument("byte_offset is not a multiple of chunk_size.");
  if (byte_length % chunk_size != 0) throw std::invalid_argument("byte_length is not a multiple of chunk_size.");
  const int chunk_offset = byte_offset / chunk_size;
  const int chunk_length = byte_length / chunk_size;
  std::vector<std::pair<Fr, Fr>> d;
  for (int i = 0; i < chunk_length; i++)
    d.push_back({Fr((long)chunk_offset + i), Fr::from_le_bytes(bytes + (size_t)i * chunk_size, chunk_size)});
  return blob(d);
}

// ---- poly -------------------------------------------------------------------
poly::poly(std::vector<Fr> _data) : data(std::move(_data)) {
  while (!data.empty() && data.back().is_zero()) data.pop_back();
}

poly poly::from_blob(blob b) {
  auto& pts = b.get_data();
  if (pts.empty()) return poly({});
  std::vector<uint64_t> xs(4 * pts.size()), ys(4 * pts.size()), c(4 * pts.size());
  for (size_t i = 0; i < pts.size(); i++) {
    std::memcpy(&xs[4 * i], pts[i].first.v.data(), 32);
    std::memcpy(&ys[4 * i], pts[i].second.v.data(), 32);
  }
  check(kzgx_poly_interpolate(default_ctx(), xs.data(), ys.data(), pts.size(), c.data()), "kzgx_poly_interpolate");
  std::vector<Fr> P(pts.size());
  for (size_t i = 0; i < pts.size(); i++) std::memcpy(P[i].v.data(), &c[4 * i], 32);
  return poly(P);
}

// ---- evaluation form (extensions) --------------------------------------------
namespace {
// log2 of a power-of-two size within the selected curve's NTT domain
unsigned domain_log2(size_t size, const char* where) {
  unsigned k = 0;
  while (((size_t)1 << k) < size) k++;
  if (size == 0 || ((size_t)1 << k) != size) throw std::invalid_argument(std::string(where) + ": size is not a power of two");
  if ((int)k > kzgx_ntt_max_log2(g_curve))
    throw std::invalid_argument(std::string(where) + ": size exceeds the curve's power-of-two domain");
  return k;
}

std::vector<Fr> unflat(const std::vector<uint64_t>& w) {
  std::vector<Fr> out(w.size() / 4);
  for (size_t i = 0; i < out.size(); i++) std::memcpy(out[i].v.data(), &w[4 * i], 32);
  return out;
}
}  // namespace

Fr domain_root(unsigned log2n) {
  Fr w;
  check(kzgx_domain_root(g_curve, log2n, w.v.data()), "kzgx_domain_root");
  return w;
}

poly poly::from_evaluations(const std::vector<Fr>& evals, bool bit_reversed) {
  const unsigned k = domain_log2(evals.size(), "from_evaluations");
  auto e = flat(evals);
  check(kzgx_ntt(default_ctx(), e.data(), k, 1, KZGX_NTT_INVERSE | (bit_reversed ? KZGX_NTT_BITREV : 0), e.data()),
        "kzgx_ntt");
  return poly(unflat(e));
}

std::vector<Fr> poly::evaluate_domain(unsigned log2n, bool bit_reversed) const {
  if ((int)log2n > kzgx_ntt_max_log2(g_curve))
    throw std::invalid_argument("evaluate_domain: size exceeds the curve's power-of-two domain");
  const size_t m = (size_t)1 << log2n;
  if (data.size() > m) throw std::invalid_argument("evaluate_domain: the polynomial has more coefficients than the domain");
  std::vector<uint64_t> c(4 * m, 0);  // zero-padded to the domain
  for (size_t i = 0; i < data.size(); i++) std::memcpy(&c[4 * i], data[i].v.data(), 32);
  check(kzgx_ntt(default_ctx(), c.data(), log2n, 1, bit_reversed ? KZGX_NTT_BITREV : 0, c.data()), "kzgx_ntt");
  return unflat(c);
}

// serialize_ZZ_pX (util.cpp:118-140): i64 degree, then per coefficient a u8
// byte count and the minimal little-endian bytes
std::vector<uint8_t> poly::serialize() {
  std::vector<uint8_t> out(8);
  int64_t d = degree();
  std::memcpy(out.data(), &d, 8);
  for (auto& c : data) {
    auto b = c.to_le_bytes();
    out.push_back((uint8_t)b.size());
    out.insert(out.end(), b.begin(), b.end());
  }
  return out;
}

poly poly::deserialize(const std::vector<uint8_t>& bytes) {
  if (bytes.size() < 8) throw std::invalid_argument("poly::deserialize: truncated");
  int64_t d;
  std::memcpy(&d, bytes.data(), 8);
  size_t off = 8;
  std::vector<Fr> P;
  for (int64_t i = 0; i <= d; i++) {
    if (off >= bytes.size()) throw std::invalid_argument("poly::deserialize: truncated");
    uint8_t nb = bytes[off++];
    if (off + nb > bytes.size()) throw std::invalid_argument("poly::deserialize: truncated");
    P.push_back(Fr::from_le_bytes(bytes.data() + off, nb));
    off += nb;
  }
  return poly(P);
}

// ---- commit / proof ---------------------------------------------------------
std::vector<uint8_t> commit::serialize() { return ecp_serialize(curve_point); }
commit commit::deserialize(const std::vector<uint8_t>& b) { return commit(ecp_deserialize(b)); }
std::vector<uint8_t> proof::serialize() { return ecp_serialize(curve_point); }
proof proof::deserialize(const std::vector<uint8_t>& b) { return proof(ecp_deserialize(b)); }

std::vector<commit> commit::deserialize_batch(const std::vector<std::vector<uint8_t>>& bytes, bool check_subgroup,
                                              std::vector<bool>* valid) {
  std::vector<commit> res;
  for (const G1& g : ecp_deserialize_batch(bytes, check_subgroup, valid)) res.push_back(commit(g));
  return res;
}

std::vector<proof> proof::deserialize_batch(const std::vector<std::vector<uint8_t>>& bytes, bool check_subgroup,
                                            std::vector<bool>* valid) {
  std::vector<proof> res;
  for (const G1& g : ecp_deserialize_batch(bytes, check_subgroup, valid)) res.push_back(proof(g));
  return res;
}

std::vector<uint8_t> commit::serialize_compressed(int encoding) { return g1_compressed(curve_point, encoding); }
std::vector<uint8_t> proof::serialize_compressed(int encoding) { return g1_compressed(curve_point, encoding); }

std::vector<commit> commit::deserialize_compressed_batch(const std::vector<uint8_t>& packed, int encoding,
                                                         bool check_subgroup, std::vector<bool>* valid) {
  std::vector<commit> res;
  for (const G1& g : g1_decompress_packed(packed, encoding, check_subgroup, valid)) res.push_back(commit(g));
  return res;
}

std::vector<proof> proof::deserialize_compressed_batch(const std::vector<uint8_t>& packed, int encoding,
                                                       bool check_subgroup, std::vector<bool>* valid) {
  std::vector<proof> res;
  for (const G1& g : g1_decompress_packed(packed, encoding, check_subgroup, valid)) res.push_back(proof(g));
  return res;
}

// ---- trusted_setup ----------------------------------------------------------
trusted_setup trusted_setup::from_compressed(const std::vector<uint8_t>& g1, const std::vector<uint8_t>& g2,
                                             bool check_subgroup) {
  const size_t r1 = record_bytes(1, KZGX_ENC_ZCASH), r2 = record_bytes(2, KZGX_ENC_ZCASH);
  if (g1.empty() || g2.empty() || g1.size() % r1 || g2.size() % r2)
    throw std::invalid_argument("from_compressed: not a whole, positive number of records");
  const size_t n1 = g1.size() / r1, n2 = g2.size() / r2;
  const int nl = base_limbs(), sg = check_subgroup ? 1 : 0;
  std::vector<uint64_t> xy(2 * nl * n1), xy2(4 * nl * n2);
  std::vector<int> inf(std::max(n1, n2)), ok(std::max(n1, n2));
  trusted_setup ts;
  check(kzgx_create(&ts.ctx, g_curve, device()), "kzgx_create");  // ts's destructor frees it on a throw
  check(kzgx_g1_decompress_batch(ts.ctx, g1.data(), n1, KZGX_ENC_ZCASH, sg, xy.data(), inf.data(), ok.data()),
        "kzgx_g1_decompress_batch");
  for (size_t i = 0; i < n1; i++)
    if (!ok[i] || inf[i]) throw std::runtime_error("bad trusted setup file");
  check(kzgx_g2_decompress_batch(ts.ctx, g2.data(), n2, sg, xy2.data(), inf.data(), ok.data()),
        "kzgx_g2_decompress_batch");
  for (size_t i = 0; i < n2; i++)
    if (!ok[i] || inf[i]) throw std::logic_error("bad trusted setup file");
  check(kzgx_load_srs_g1(ts.ctx, xy.data(), n1), "kzgx_load_srs_g1");
  check(kzgx_load_srs_g2(ts.ctx, xy2.data(), n2), "kzgx_load_srs_g2");
  ts.n = n1;
  return ts;
}

trusted_setup::trusted_setup(int num_coeff) {
  if (num_coeff < 2) throw std::invalid_argument("num_coeff must be at least 2");
  // generate_random_BIG (util.cpp:62-76): 32 bytes from std::random_device, mod r
  std::random_device rd;
  uint8_t seed[32];
  for (auto& b : seed) b = (uint8_t)rd();
  Fr tau = Fr::from_le_bytes(seed, 32);
  check(kzgx_create(&ctx, g_curve, device()), "kzgx_create");
  check(kzgx_gen_srs_g1(ctx, tau.v.data(), 0, (size_t)num_coeff), "kzgx_gen_srs_g1");
  check(kzgx_gen_srs_g2(ctx, tau.v.data(), 0, (size_t)num_coeff), "kzgx_gen_srs_g2");
  n = (size_t)num_coeff;
  tau.v.fill(0);
  std::memset(seed, 0, sizeof seed);  // tau is toxic waste; the reference discards it too
}

trusted_setup::trusted_setup(int num_coeff, const Fr& tau) {
  if (num_coeff < 2) throw std::invalid_argument("num_coeff must be at least 2");
  check(kzgx_create(&ctx, g_curve, device()), "kzgx_create");
  check(kzgx_gen_srs_g1(ctx, tau.v.data(), 0, (size_t)num_coeff), "kzgx_gen_srs_g1");
  check(kzgx_gen_srs_g2(ctx, tau.v.data(), 0, (size_t)num_coeff), "kzgx_gen_srs_g2");
  n = (size_t)num_coeff;
}

trusted_setup::trusted_setup(const std::string& filename) {
  std::ifstream f(filename, std::ios::in | std::ios::binary);
  if (!f.is_open()) throw std::runtime_error("could not open trusted setup file");
  uint64_t num = 0;
  f.read(reinterpret_cast<char*>(&num), 8);
  if (!f || num == 0 || num > (1ull << 31)) throw std::runtime_error("bad trusted setup file");
  const size_t mb = mod_bytes();
  const int nl = base_limbs();
  std::vector<uint64_t> xy(2 * nl * num, 0);
  std::vector<uint8_t> one;
  for (uint64_t i = 0; i < num; i++) {
    uint32_t len = 0;
    f.read(reinterpret_cast<char*>(&len), 4);
    // the reference reads len bytes into a fixed buffer without a check
    // (trusted_setup.cpp:93-94); we reject anything but the uncompressed octet
    if (!f || len != 1 + 2 * mb) throw std::runtime_error("bad trusted setup file");
    std::vector<uint8_t> rec(4 + len);
    std::memcpy(rec.data(), &len, 4);
    f.read(reinterpret_cast<char*>(rec.data() + 4), len);
    if (!f) throw std::runtime_error("bad trusted setup file");
    G1 g = ecp_deserialize(rec);
    if (g.inf) throw std::runtime_error("bad trusted setup file");
    for (int k = 0; k < nl; k++) {
      xy[2 * nl * i + k] = g.x[k];
      xy[2 * nl * i + nl + k] = g.y[k];
    }
  }
  // G2 records (trusted_setup.cpp:103-118); a bad one is a logic_error there
  std::vector<uint64_t> xy2(4 * nl * num, 0);
  for (uint64_t i = 0; i < num; i++) {
    uint32_t len = 0;
    f.read(reinterpret_cast<char*>(&len), 4);
    if (!f || len != 1 + 4 * mb) throw std::logic_error("bad trusted setup file");
    std::vector<uint8_t> oct(len);
    f.read(reinterpret_cast<char*>(oct.data()), len);
    if (!f || oct[0] != 0x04) throw std::logic_error("bad trusted setup file");
    uint64_t* w = &xy2[4 * nl * i];
    get_be(&oct[1], w + nl, mb);           // x.im
    get_be(&oct[1 + mb], w, mb);           // x.re
    get_be(&oct[1 + 2 * mb], w + 3 * nl, mb);  // y.im
    get_be(&oct[1 + 3 * mb], w + 2 * nl, mb);  // y.re
  }
  check(kzgx_create(&ctx, g_curve, device()), "kzgx_create");
  std::vector<int> ok(num, 0);
  check(kzgx_g2_validate(ctx, xy2.data(), num, ok.data()), "kzgx_g2_validate");
  for (uint64_t i = 0; i < num; i++)
    if (!ok[i]) {
      kzgx_destroy(ctx);
      ctx = nullptr;
      throw std::logic_error("bad trusted setup file");
    }
  check(kzgx_load_srs_g1(ctx, xy.data(), num), "kzgx_load_srs_g1");
  check(kzgx_load_srs_g2(ctx, xy2.data(), num), "kzgx_load_srs_g2");
  n = num;
}

trusted_setup::~trusted_setup() {
  if (ctx) kzgx_destroy(ctx);
}

trusted_setup::trusted_setup(trusted_setup&& o) noexcept : ctx(o.ctx), n(o.n) {
  o.ctx = nullptr;
  o.n = 0;
}

trusted_setup& trusted_setup::operator=(trusted_setup&& o) noexcept {
  if (this != &o) {
    if (ctx) kzgx_destroy(ctx);
    ctx = o.ctx;
    n = o.n;
    o.ctx = nullptr;
    o.n = 0;
  }
  return *this;
}

G1 trusted_setup::polyeval_G1(const std::vector<Fr>& P) {
  if (P.empty()) return G1();  // deg -1 -> ECP_inf (trusted_setup.cpp:150-154)
  auto s = flat(P);
  std::vector<uint64_t> out(2 * base_limbs());
  int inf = 1;
  check(kzgx_msm_g1(ctx, s.data(), P.size(), out.data(), &inf), "kzgx_msm_g1");
  return to_g1(out.data(), inf);
}

commit trusted_setup::create_commit(const kzg::poly& p) {
  if (p.degree() + 1 >= (long)n)
    throw std::invalid_argument("polynomial degree be at most one less than the setup size (num_coeffs)");
  return commit(polyeval_G1(p.get_poly()));
}

bool trusted_setup::verify_commit(kzg::commit& c, const kzg::poly& p) {
  commit expected = create_commit(p);
  return c.get_curve_point() == expected.get_curve_point();
}

proof trusted_setup::create_proof(const kzg::poly& p, int byte_offset, int byte_length, int chunk_size) {
  if (chunk_size > MAX_CHUNK_BYTES) throw std::invalid_argument("chunk_size must at most MAX_CHUNK_BYTES.");
  if (chunk_size < 1) throw std::invalid_argument("chunk_size must be at least 1.");
  if (byte_offset % chunk_size != 0) throw std::invalid_argument("byte_offset is not a multiple of chunk_size.");
  if (byte_length % chunk_size != 0) throw std::invalid_argument("byte_length is not a multiple of chun_size.");
  return create_proof(p, byte_offset / chunk_size, byte_length / chunk_size);
}

proof trusted_setup::create_proof(const kzg::poly& p, int chunk_offset, int chunk_length) {
  if (chunk_length < 1) throw std::invalid_argument("chunk_length must be 1 or greater");
  const auto& P = p.get_poly();
  // the reference reads past _G1 here (UB) when deg q >= size; we refuse
  if ((long)P.size() - chunk_length > (long)n)
    throw std::invalid_argument("polynomial degree be at most one less than the setup size (num_coeffs)");
  auto c = flat(P);
  std::vector<uint64_t> out(2 * base_limbs());
  int inf = 1;
  if (chunk_length == 1) {
    Fr z((long)chunk_offset);
    uint64_t y[4];
    if (P.empty()) return proof(G1());
    check(kzgx_prove_single_batch(ctx, c.data(), P.size(), 0, z.v.data(), 1, out.data(), &inf, y),
          "kzgx_prove_single_batch");
    return proof(to_g1(out.data(), inf));
  }
  std::vector<uint64_t> xs(4 * (size_t)chunk_length);
  for (int i = 0; i < chunk_length; i++) {
    Fr x((long)chunk_offset + i);
    std::memcpy(&xs[4 * (size_t)i], x.v.data(), 32);
  }
  check(kzgx_prove_range(ctx, P.empty() ? nullptr : c.data(), P.size(), xs.data(), (size_t)chunk_length, out.data(),
                         &inf),
        "kzgx_prove_range");
  return proof(to_g1(out.data(), inf));
}

bool trusted_setup::verify_proof(commit& c, proof& pf, blob& expected_data) {
  auto& pts = expected_data.get_data();
  if (pts.size() < 1) throw std::invalid_argument("expected_data size must be 1 or greater");
  if (pts.size() >= n) return false;
  const int nl = base_limbs();
  std::vector<uint64_t> cxy(2 * nl, 0), pxy(2 * nl, 0), xs(4 * pts.size()), ys(4 * pts.size());
  const G1& cg = c.get_curve_point();
  const G1& pg = pf.get_curve_point();
  for (int i = 0; i < nl; i++) {
    cxy[i] = cg.x[i];
    cxy[nl + i] = cg.y[i];
    pxy[i] = pg.x[i];
    pxy[nl + i] = pg.y[i];
  }
  for (size_t j = 0; j < pts.size(); j++) {
    std::memcpy(&xs[4 * j], pts[j].first.v.data(), 32);
    std::memcpy(&ys[4 * j], pts[j].second.v.data(), 32);
  }
  int ok = 0;
  check(kzgx_verify_proof(ctx, cxy.data(), cg.inf ? 1 : 0, pxy.data(), pg.inf ? 1 : 0, xs.data(), ys.data(),
                          pts.size(), &ok),
        "kzgx_verify_proof");
  return ok != 0;
}

void trusted_setup::export_setup(const std::string& filename) {
  std::ofstream file(filename, std::ios::out | std::ios::binary | std::ios::trunc);
  if (!file.is_open()) {
    std::cerr << "failed to export" << std::endl;
    return;
  }
  const uint64_t num = n;
  file.write(reinterpret_cast<const char*>(&num), 8);
  for (const G1& g : g1_points()) {
    auto rec = ecp_serialize(g);  // u32 len || octet
    file.write(reinterpret_cast<const char*>(rec.data()), (std::streamsize)rec.size());
  }
  for (const G2& g : g2_points()) {
    auto oct = ecp2_octet(g);
    const uint32_t len = (uint32_t)oct.size();
    file.write(reinterpret_cast<const char*>(&len), 4);
    file.write(reinterpret_cast<const char*>(oct.data()), (std::streamsize)oct.size());
  }
}

std::vector<commit> trusted_setup::create_commits(const std::vector<kzg::poly>& polys) {
  std::vector<commit> res;
  if (polys.empty()) return res;
  size_t m = 0;
  for (auto& p : polys) {
    if (p.degree() + 1 >= (long)n)
      throw std::invalid_argument("polynomial degree be at most one less than the setup size (num_coeffs)");
    m = std::max(m, p.get_poly().size());
  }
  if (m == 0) return std::vector<commit>(polys.size(), commit(G1()));
  std::vector<uint64_t> s(4 * m * polys.size(), 0);  // zero-padded to a common length
  for (size_t b = 0; b < polys.size(); b++) {
    auto f = flat(polys[b].get_poly());
    std::memcpy(&s[4 * m * b], f.data(), f.size() * 8);
  }
  const int nl = base_limbs();
  std::vector<uint64_t> out(2 * nl * polys.size());
  std::vector<int> inf(polys.size());
  check(kzgx_msm_g1_batch(ctx, s.data(), m, polys.size(), out.data(), inf.data()), "kzgx_msm_g1_batch");
  for (size_t b = 0; b < polys.size(); b++) res.push_back(commit(to_g1(&out[2 * nl * b], inf[b])));
  return res;
}

std::vector<proof> trusted_setup::create_proofs(const kzg::poly& p, const std::vector<long>& points) {
  std::vector<proof> res;
  const auto& P = p.get_poly();
  if (points.empty()) return res;
  if (P.empty()) return std::vector<proof>(points.size(), proof(G1()));
  if ((long)P.size() - 1 > (long)n)
    throw std::invalid_argument("polynomial degree be at most one less than the setup size (num_coeffs)");
  auto c = flat(P);
  std::vector<uint64_t> zs(4 * points.size());
  for (size_t j = 0; j < points.size(); j++) {
    Fr z(points[j]);
    std::memcpy(&zs[4 * j], z.v.data(), 32);
  }
  const int nl = base_limbs();
  std::vector<uint64_t> out(2 * nl * points.size());
  std::vector<int> inf(points.size());
  check(kzgx_prove_single_batch(ctx, c.data(), P.size(), 0, zs.data(), points.size(), out.data(), inf.data(),
                                nullptr),
        "kzgx_prove_single_batch");
  for (size_t j = 0; j < points.size(); j++) res.push_back(proof(to_g1(&out[2 * nl * j], inf[j])));
  return res;
}

std::vector<commit> trusted_setup::create_commits_from_evaluations(const std::vector<std::vector<Fr>>& evals,
                                                                   bool bit_reversed) {
  std::vector<commit> res;
  if (evals.empty()) return res;
  const size_t m = evals[0].size();
  const unsigned k = domain_log2(m, "create_commits_from_evaluations");
  for (auto& e : evals)
    if (e.size() != m) throw std::invalid_argument("create_commits_from_evaluations: vectors of different sizes");
  if (m >= n) throw std::invalid_argument("the domain must be smaller than the setup size (num_coeffs)");
  std::vector<uint64_t> s(4 * m * evals.size());
  for (size_t b = 0; b < evals.size(); b++) std::memcpy(&s[4 * m * b], flat(evals[b]).data(), 32 * m);
  const int nl = base_limbs();
  std::vector<uint64_t> out(2 * nl * evals.size());
  std::vector<int> inf(evals.size());
  check(kzgx_commit_evals_batch(ctx, s.data(), k, evals.size(), bit_reversed ? KZGX_NTT_BITREV : 0, out.data(),
                                inf.data()),
        "kzgx_commit_evals_batch");
  for (size_t b = 0; b < evals.size(); b++) res.push_back(commit(to_g1(&out[2 * nl * b], inf[b])));
  return res;
}

std::vector<proof> trusted_setup::create_proofs_from_evaluations(const std::vector<Fr>& evals,
                                                                const std::vector<Fr>& points, bool bit_reversed) {
  std::vector<proof> res;
  const unsigned k = domain_log2(evals.size(), "create_proofs_from_evaluations");
  if (evals.size() >= n) throw std::invalid_argument("the domain must be smaller than the setup size (num_coeffs)");
  if (points.empty()) return res;
  auto e = flat(evals), zs = flat(points);
  const int nl = base_limbs();
  std::vector<uint64_t> out(2 * nl * points.size());
  std::vector<int> inf(points.size());
  check(kzgx_prove_evals_batch(ctx, e.data(), k, 0, zs.data(), points.size(), bit_reversed ? KZGX_NTT_BITREV : 0,
                               out.data(), inf.data(), nullptr),
        "kzgx_prove_evals_batch");
  for (size_t j = 0; j < points.size(); j++) res.push_back(proof(to_g1(&out[2 * nl * j], inf[j])));
  return res;
}

// the all-domain openings of one polynomial: in = 2^k scalars, coefficients or values
static std::vector<proof> all_proofs(kzgx_ctx* ctx, size_t n, const std::vector<uint64_t>& in, unsigned k, int flags) {
  if ((int)k + 1 > kzgx_ntt_max_log2(g_curve))
    throw std::invalid_argument("all proofs: the twice larger domain exceeds the curve's power-of-two domain");
  const size_t m = (size_t)1 << k;
  if (m >= n) throw std::invalid_argument("the domain must be smaller than the setup size (num_coeffs)");
  const int nl = base_limbs();
  std::vector<uint64_t> out(2 * nl * m);
  std::vector<int> inf(m);
  check(kzgx_prove_all_batch(ctx, in.data(), k, 1, flags, out.data(), inf.data(), nullptr), "kzgx_prove_all_batch");
  std::vector<proof> res;
  for (size_t j = 0; j < m; j++) res.push_back(proof(to_g1(&out[2 * nl * j], inf[j])));
  return res;
}

std::vector<proof> trusted_setup::create_all_proofs(const kzg::poly& p, unsigned log2n, bool bit_reversed) {
  if ((int)log2n > kzgx_ntt_max_log2(g_curve))
    throw std::invalid_argument("create_all_proofs: size exceeds the curve's power-of-two domain");
  const auto& P = p.get_poly();
  const size_t m = (size_t)1 << log2n;
  if (P.size() > m) throw std::invalid_argument("create_all_proofs: the polynomial has more coefficients than the domain");
  std::vector<uint64_t> c(4 * m, 0);  // zero-padded to the domain
  for (size_t i = 0; i < P.size(); i++) std::memcpy(&c[4 * i], P[i].v.data(), 32);
  return all_proofs(ctx, n, c, log2n, bit_reversed ? KZGX_NTT_BITREV : 0);
}

std::vector<proof> trusted_setup::create_all_proofs_from_evaluations(const std::vector<Fr>& evals, bool bit_reversed) {
  const unsigned k = domain_log2(evals.size(), "create_all_proofs_from_evaluations");
  return all_proofs(ctx, n, flat(evals), k, KZGX_PROVE_ALL_EVALS | (bit_reversed ? KZGX_NTT_BITREV : 0));
}

// the coset openings of one polynomial: in = 2^k scalars, coefficients or values
static std::vector<proof> coset_proofs(kzgx_ctx* ctx, size_t n, const std::vector<uint64_t>& in, unsigned k,
                                       unsigned kl, int flags) {
  const int mx = kzgx_ntt_max_log2(g_curve), ext = (flags & KZGX_PROVE_COSETS_EXTENDED) ? 1 : 0;
  if (kl > k) throw std::invalid_argument("coset proofs: a coset larger than the domain");
  if ((int)(k - kl) + 1 > mx || (int)k + ext > mx)
    throw std::invalid_argument("coset proofs: a domain the shape needs exceeds the curve's power-of-two domain");
  const size_t m = (size_t)1 << k, R = (size_t)1 << (k - kl + ext);
  if (m >= n) throw std::invalid_argument("the domain must be smaller than the setup size (num_coeffs)");
  const int nl = base_limbs();
  std::vector<uint64_t> out(2 * nl * R);
  std::vector<int> inf(R);
  check(kzgx_prove_cosets_batch(ctx, in.data(), k, kl, 1, flags, out.data(), inf.data(), nullptr),
        "kzgx_prove_cosets_batch");
  std::vector<proof> res;
  for (size_t j = 0; j < R; j++) res.push_back(proof(to_g1(&out[2 * nl * j], inf[j])));
  return res;
}

std::vector<proof> trusted_setup::create_coset_proofs(const kzg::poly& p, unsigned log2n, unsigned log2l, bool extended,
                                                      bool bit_reversed) {
  if ((int)log2n > kzgx_ntt_max_log2(g_curve))
    throw std::invalid_argument("create_coset_proofs: size exceeds the curve's power-of-two domain");
  const auto& P = p.get_poly();
  const size_t m = (size_t)1 << log2n;
  if (P.size() > m)
    throw std::invalid_argument("create_coset_proofs: the polynomial has more coefficients than the domain");
  std::vector<uint64_t> c(4 * m, 0);  // zero-padded to the domain
  for (size_t i = 0; i < P.size(); i++) std::memcpy(&c[4 * i], P[i].v.data(), 32);
  return coset_proofs(ctx, n, c, log2n, log2l,
                      (extended ? KZGX_PROVE_COSETS_EXTENDED : 0) | (bit_reversed ? KZGX_NTT_BITREV : 0));
}

std::vector<proof> trusted_setup::create_coset_proofs_from_evaluations(const std::vector<Fr>& evals, unsigned log2l,
                                                                      bool extended, bool bit_reversed) {
  const unsigned k = domain_log2(evals.size(), "create_coset_proofs_from_evaluations");
  return coset_proofs(ctx, n, flat(evals), k, log2l,
                      KZGX_PROVE_ALL_EVALS | (extended ? KZGX_PROVE_COSETS_EXTENDED : 0) |
                          (bit_reversed ? KZGX_NTT_BITREV : 0));
}

std::vector<bool> trusted_setup::verify_proofs(std::vector<commit>& commits, std::vector<proof>& proofs,
                                              const std::vector<std::pair<Fr, Fr>>& points) {
  const size_t m = commits.size();
  if (proofs.size() != m || points.size() != m) throw std::invalid_argument("verify_proofs: size mismatch");
  std::vector<bool> res(m, false);
  if (m == 0) return res;
  const int nl = base_limbs();
  std::vector<uint64_t> c(2 * nl * m, 0), p(2 * nl * m, 0), z(4 * m), y(4 * m);
  std::vector<int> ci(m), pi(m), ok(m);
  for (size_t k = 0; k < m; k++) {
    const G1& cg = commits[k].get_curve_point();
    const G1& pg = proofs[k].get_curve_point();
    for (int i = 0; i < nl; i++) {
      c[2 * nl * k + i] = cg.x[i];
      c[2 * nl * k + nl + i] = cg.y[i];
      p[2 * nl * k + i] = pg.x[i];
      p[2 * nl * k + nl + i] = pg.y[i];
    }
    ci[k] = cg.inf;
    pi[k] = pg.inf;
    std::memcpy(&z[4 * k], points[k].first.v.data(), 32);
    std::memcpy(&y[4 * k], points[k].second.v.data(), 32);
  }
  check(kzgx_verify_single_batch(ctx, c.data(), ci.data(), p.data(), pi.data(), z.data(), y.data(), m, ok.data()),
        "kzgx_verify_single_batch");
  for (size_t k = 0; k < m; k++) res[k] = ok[k] != 0;
  return res;
}

bool trusted_setup::verify_proofs_aggregated(std::vector<commit>& commits, std::vector<proof>& proofs,
                                             const std::vector<std::pair<Fr, Fr>>& points) {
  return aggregated(commits, proofs, points, false, false);
}

bool trusted_setup::verify_proofs_aggregated(std::vector<commit>& commits, std::vector<proof>& proofs,
                                             const std::vector<std::pair<Fr, Fr>>& points, bool check_subgroup) {
  return aggregated(commits, proofs, points, true, check_subgroup);
}

bool trusted_setup::check_setup(bool subgroup) {
  int g1_ok = 0, g2_ok = 0;
  check(kzgx_srs_check(ctx, subgroup ? 1 : 0, &g1_ok, &g2_ok), "kzgx_srs_check");
  return g1_ok != 0 && g2_ok != 0;
}

G2 trusted_setup::contribute(const Fr& s) {
  const int nl = base_limbs();
  std::vector<uint64_t> w(4 * nl, 0);
  check(kzgx_srs_update(ctx, s.v.data(), 0, 0, w.data()), "kzgx_srs_update");
  return to_g2(w.data(), false);  // s != 0: the witness is finite
}

bool trusted_setup::verify_structure(bool generators) {
  int g1_ok = 0, g2_ok = 0;
  check(kzgx_srs_verify_structure(ctx, nullptr, nullptr, generators ? KZGX_SRS_STRUCT_GENERATORS : 0, &g1_ok, &g2_ok),
        "kzgx_srs_verify_structure");
  return g1_ok != 0 && g2_ok != 0;
}

bool trusted_setup::verify_contribution(const G1& prev_tau, const G1& new_tau, const G2& witness) {
  const int nl = base_limbs();
  std::vector<uint64_t> p(2 * nl, 0), q(2 * nl, 0), w(4 * nl, 0);  // infinity = all zero
  for (int i = 0; i < nl; i++) {
    if (!prev_tau.inf) p[i] = prev_tau.x[i], p[nl + i] = prev_tau.y[i];
    if (!new_tau.inf) q[i] = new_tau.x[i], q[nl + i] = new_tau.y[i];
    if (!witness.inf)
      w[i] = witness.x0[i], w[nl + i] = witness.x1[i], w[2 * nl + i] = witness.y0[i], w[3 * nl + i] = witness.y1[i];
  }
  int ok = 0;
  check(kzgx_srs_verify_update(default_ctx(), p.data(), q.data(), w.data(), &ok), "kzgx_srs_verify_update");
  return ok != 0;
}

bool trusted_setup::aggregated(std::vector<commit>& commits, std::vector<proof>& proofs,
                               const std::vector<std::pair<Fr, Fr>>& points, bool checked, bool check_subgroup) {
  const size_t m = commits.size();
  if (proofs.size() != m || points.size() != m)
    throw std::invalid_argument("verify_proofs_aggregated: size mismatch");
  if (m == 0) return true;
  const int nl = base_limbs();
  std::vector<uint64_t> c(2 * nl * m, 0), p(2 * nl * m, 0), z(4 * m), y(4 * m);
  std::vector<int> ci(m), pi(m);
  for (size_t k = 0; k < m; k++) {
    const G1& cg = commits[k].get_curve_point();
    const G1& pg = proofs[k].get_curve_point();
    for (int i = 0; i < nl; i++) {
      c[2 * nl * k + i] = cg.x[i];
      c[2 * nl * k + nl + i] = cg.y[i];
      p[2 * nl * k + i] = pg.x[i];
      p[2 * nl * k + nl + i] = pg.y[i];
    }
    ci[k] = cg.inf;
    pi[k] = pg.inf;
    std::memcpy(&z[4 * k], points[k].first.v.data(), 32);
    std::memcpy(&y[4 * k], points[k].second.v.data(), 32);
  }
  int ok = 0;
  if (checked)
    check(kzgx_verify_aggregate_checked(ctx, c.data(), ci.data(), p.data(), pi.data(), z.data(), y.data(), nullptr, m,
                                        check_subgroup ? 1 : 0, &ok),
          "kzgx_verify_aggregate_checked");
  else
    check(kzgx_verify_aggregate(ctx, c.data(), ci.data(), p.data(), pi.data(), z.data(), y.data(), nullptr, m, &ok),
          "kzgx_verify_aggregate");
  return ok != 0;
}

bool trusted_setup::verify_coset_proofs(std::vector<commit>& commits, const std::vector<uint32_t>& commit_index,
                                        const std::vector<uint32_t>& cell_index, std::vector<proof>& proofs,
                                        const std::vector<std::vector<Fr>>& values, unsigned log2n, bool extended,
                                        bool bit_reversed) {
  return coset_aggregated(commits, commit_index, cell_index, proofs, values, log2n, extended, bit_reversed, false,
                          false);
}

bool trusted_setup::verify_coset_proofs(std::vector<commit>& commits, const std::vector<uint32_t>& commit_index,
                                        const std::vector<uint32_t>& cell_index, std::vector<proof>& proofs,
                                        const std::vector<std::vector<Fr>>& values, unsigned log2n, bool extended,
                                        bool bit_reversed, bool check_subgroup) {
  return coset_aggregated(commits, commit_index, cell_index, proofs, values, log2n, extended, bit_reversed, true,
                          check_subgroup);
}

std::vector<bool> trusted_setup::verify_coset_proofs_each(std::vector<commit>& commits,
                                                          const std::vector<uint32_t>& commit_index,
                                                          const std::vector<uint32_t>& cell_index,
                                                          std::vector<proof>& proofs,
                                                          const std::vector<std::vector<Fr>>& values, unsigned log2n,
                                                          bool extended, bool bit_reversed) {
  std::vector<bool> each;
  coset_aggregated(commits, commit_index, cell_index, proofs, values, log2n, extended, bit_reversed, false, false,
                   &each);
  return each;
}

std::vector<bool> trusted_setup::verify_coset_proofs_each(std::vector<commit>& commits,
                                                          const std::vector<uint32_t>& commit_index,
                                                          const std::vector<uint32_t>& cell_index,
                                                          std::vector<proof>& proofs,
                                                          const std::vector<std::vector<Fr>>& values, unsigned log2n,
                                                          bool extended, bool bit_reversed, bool check_subgroup) {
  std::vector<bool> each;
  coset_aggregated(commits, commit_index, cell_index, proofs, values, log2n, extended, bit_reversed, true,
                   check_subgroup, &each);
  return each;
}

// the argument checks of the cell verifies (m cells of nc commitments); log2 of the cell size, 0 for m = 0
static unsigned coset_cells_log2l(size_t m, size_t nc, const std::vector<uint32_t>& commit_index,
                                  const std::vector<uint32_t>& cell_index, const std::vector<std::vector<Fr>>& values,
                                  unsigned log2n, bool extended) {
  if (commit_index.size() != m || cell_index.size() != m || values.size() != m)
    throw std::invalid_argument("verify_coset_proofs: size mismatch");
  if (m == 0) return 0;
  const size_t l = values[0].size();
  if (l == 0 || (l & (l - 1))) throw std::invalid_argument("verify_coset_proofs: a cell's size is not a power of two");
  unsigned kl = 0;
  while (((size_t)1 << kl) < l) kl++;
  const int mx = kzgx_ntt_max_log2(g_curve), ext = extended ? 1 : 0;
  if (kl > log2n) throw std::invalid_argument("verify_coset_proofs: a coset larger than the domain");
  if (log2n > 31 || (int)log2n + ext > mx)
    throw std::invalid_argument("verify_coset_proofs: the opened domain exceeds the curve's power-of-two domain");
  const size_t R = (size_t)1 << (log2n - kl + ext);
  for (size_t k = 0; k < m; k++) {
    if (values[k].size() != l) throw std::invalid_argument("verify_coset_proofs: cells of different sizes");
    if (commit_index[k] >= nc || cell_index[k] >= R)
      throw std::invalid_argument("verify_coset_proofs: index out of range");
  }
  return kl;
}

bool trusted_setup::verify_coset_proofs(const std::vector<uint8_t>& commits, const std::vector<uint32_t>& commit_index,
                                        const std::vector<uint32_t>& cell_index, const std::vector<uint8_t>& proofs,
                                        const std::vector<std::vector<Fr>>& values, unsigned log2n, bool extended,
                                        bool bit_reversed, int encoding, bool check_subgroup) {
  const size_t rb = record_bytes(1, encoding);
  if (commits.size() % rb || proofs.size() % rb)
    throw std::invalid_argument("verify_coset_proofs: not a whole number of records");
  const size_t m = proofs.size() / rb, nc = commits.size() / rb;
  const unsigned kl = coset_cells_log2l(m, nc, commit_index, cell_index, values, log2n, extended);
  if (m == 0) return true;
  const size_t l = values[0].size();
  std::vector<uint64_t> y(4 * m * l);
  for (size_t k = 0; k < m; k++)
    for (size_t j = 0; j < l; j++) std::memcpy(&y[4 * (k * l + j)], values[k][j].v.data(), 32);
  const int flags = (extended ? KZGX_PROVE_COSETS_EXTENDED : 0) | (bit_reversed ? KZGX_NTT_BITREV : 0);
  int ok = 0;
  check(kzgx_verify_cells_aggregate_bytes(ctx, commits.data(), nc, commit_index.data(), cell_index.data(),
                                          proofs.data(), y.data(), nullptr, m, log2n, kl, flags, encoding,
                                          check_subgroup ? 1 : 0, &ok),
        "kzgx_verify_cells_aggregate_bytes");
  return ok != 0;
}

bool trusted_setup::coset_aggregated(std::vector<commit>& commits, const std::vector<uint32_t>& commit_index,
                                     const std::vector<uint32_t>& cell_index, std::vector<proof>& proofs,
                                     const std::vector<std::vector<Fr>>& values, unsigned log2n, bool extended,
                                     bool bit_reversed, bool checked, bool check_subgroup,
                                     std::vector<bool>* each) {
  // each: one verdict per cell (kzgx_verify_cells_each*) instead of the aggregate's one answer
  const size_t m = proofs.size(), nc = commits.size();
  const unsigned kl = coset_cells_log2l(m, nc, commit_index, cell_index, values, log2n, extended);
  if (each) each->clear();
  if (m == 0) return true;
  const size_t l = values[0].size();
  const int nl = base_limbs();
  std::vector<uint64_t> c(2 * nl * nc, 0), p(2 * nl * m, 0), y(4 * m * l);
  std::vector<int> ci(nc), pi(m);
  for (size_t k = 0; k < nc; k++) {
    const G1& cg = commits[k].get_curve_point();
    for (int i = 0; i < nl; i++) {
      c[2 * nl * k + i] = cg.x[i];
      c[2 * nl * k + nl + i] = cg.y[i];
    }
    ci[k] = cg.inf;
  }
  for (size_t k = 0; k < m; k++) {
    const G1& pg = proofs[k].get_curve_point();
    for (int i = 0; i < nl; i++) {
      p[2 * nl * k + i] = pg.x[i];
      p[2 * nl * k + nl + i] = pg.y[i];
    }
    pi[k] = pg.inf;
    for (size_t j = 0; j < l; j++) std::memcpy(&y[4 * (k * l + j)], values[k][j].v.data(), 32);
  }
  const int flags = (extended ? KZGX_PROVE_COSETS_EXTENDED : 0) | (bit_reversed ? KZGX_NTT_BITREV : 0);
  if (each) {
    std::vector<int> oks(m, 0);
    if (checked)
      check(kzgx_verify_cells_each_checked(ctx, c.data(), ci.data(), nc, commit_index.data(), cell_index.data(),
                                           p.data(), pi.data(), y.data(), m, log2n, kl, flags, check_subgroup ? 1 : 0,
                                           oks.data()),
            "kzgx_verify_cells_each_checked");
    else
      check(kzgx_verify_cells_each(ctx, c.data(), ci.data(), nc, commit_index.data(), cell_index.data(), p.data(),
                                   pi.data(), y.data(), m, log2n, kl, flags, oks.data()),
            "kzgx_verify_cells_each");
    bool all = true;
    for (int v : oks) {
      each->push_back(v != 0);
      all = all && v != 0;
    }
    return all;
  }
  int ok = 0;
  if (checked)
    check(kzgx_verify_cells_aggregate_checked(ctx, c.data(), ci.data(), nc, commit_index.data(), cell_index.data(),
                                              p.data(), pi.data(), y.data(), nullptr, m, log2n, kl, flags,
                                              check_subgroup ? 1 : 0, &ok),
          "kzgx_verify_cells_aggregate_checked");
  else
    check(kzgx_verify_cells_aggregate(ctx, c.data(), ci.data(), nc, commit_index.data(), cell_index.data(), p.data(),
                                      pi.data(), y.data(), nullptr, m, log2n, kl, flags, &ok),
          "kzgx_verify_cells_aggregate");
  return ok != 0;
}

// one blob through kzgx_recover_cells(_and_proofs): the D values, and the R proofs when asked for
std::vector<Fr> trusted_setup::recovered(const std::vector<uint32_t>& cell_index,
                                         const std::vector<std::vector<Fr>>& values, unsigned log2n,
                                         bool bit_reversed, std::vector<proof>* proofs) {
  const size_t m = cell_index.size();
  if (values.size() != m) throw std::invalid_argument("recover_cells: size mismatch");
  if (m == 0) throw std::invalid_argument("recover_cells: no cells");
  const size_t l = values[0].size();
  if (l == 0 || (l & (l - 1))) throw std::invalid_argument("recover_cells: a cell's size is not a power of two");
  unsigned kl = 0;
  while (((size_t)1 << kl) < l) kl++;
  if (kl > log2n) throw std::invalid_argument("recover_cells: a coset larger than the domain");
  if (log2n > 31 || (int)log2n + 1 > kzgx_ntt_max_log2(g_curve))
    throw std::invalid_argument("recover_cells: the extended domain exceeds the curve's power-of-two domain");
  if (log2n + 1 - kl > KZGX_RECOVER_MAX_LOG2_CELLS) throw std::invalid_argument("recover_cells: too many cells");
  const size_t D = (size_t)2 << log2n, R = D >> kl;
  if (proofs && D / 2 >= n) throw std::invalid_argument("the domain must be smaller than the setup size (num_coeffs)");
  if (m < R / 2) throw std::invalid_argument("recover_cells: fewer than half the cells");
  std::vector<bool> seen(R, false);
  std::vector<uint64_t> y(4 * m * l), out(4 * D);
  for (size_t k = 0; k < m; k++) {
    if (values[k].size() != l) throw std::invalid_argument("recover_cells: cells of different sizes");
    if (cell_index[k] >= R) throw std::invalid_argument("recover_cells: index out of range");
    if (seen[cell_index[k]]) throw std::invalid_argument("recover_cells: a cell given twice");
    seen[cell_index[k]] = true;
    for (size_t j = 0; j < l; j++) std::memcpy(&y[4 * (k * l + j)], values[k][j].v.data(), 32);
  }
  const std::vector<uint32_t> blob(m, 0);
  const int flags = KZGX_PROVE_COSETS_EXTENDED | (bit_reversed ? KZGX_NTT_BITREV : 0);
  int ok = 0;
  if (proofs) {
    const int nl = base_limbs();
    std::vector<uint64_t> pxy(2 * nl * R);
    std::vector<int> inf(R);
    check(kzgx_recover_cells_and_proofs(ctx, blob.data(), cell_index.data(), y.data(), m, 1, log2n, kl, flags,
                                        out.data(), nullptr, pxy.data(), inf.data(), &ok),
          "kzgx_recover_cells_and_proofs");
    proofs->clear();
    for (size_t j = 0; j < R; j++) proofs->push_back(proof(to_g1(&pxy[2 * nl * j], inf[j])));
  } else {
    check(kzgx_recover_cells(ctx, blob.data(), cell_index.data(), y.data(), m, 1, log2n, kl, flags, out.data(),
                             nullptr, &ok),
          "kzgx_recover_cells");
  }
  if (!ok) throw std::domain_error("recover_cells: the cells lie on no polynomial of fewer than 2^log2n coefficients");
  std::vector<Fr> res(D);
  for (size_t i = 0; i < D; i++) std::memcpy(res[i].v.data(), &out[4 * i], 32);
  return res;
}

std::vector<Fr> trusted_setup::recover_cells(const std::vector<uint32_t>& cell_index,
                                             const std::vector<std::vector<Fr>>& values, unsigned log2n,
                                             bool bit_reversed) {
  return recovered(cell_index, values, log2n, bit_reversed, nullptr);
}

std::pair<std::vector<Fr>, std::vector<proof>> trusted_setup::recover_cells_and_proofs(
    const std::vector<uint32_t>& cell_index, const std::vector<std::vector<Fr>>& values, unsigned log2n,
    bool bit_reversed) {
  std::vector<proof> proofs;
  std::vector<Fr> y = recovered(cell_index, values, log2n, bit_reversed, &proofs);
  return {std::move(y), std::move(proofs)};
}

namespace {
// blobs of 2^log2n 32-byte elements back to back: how many
size_t blob_count(const std::vector<uint8_t>& blobs, unsigned log2n, const char* where) {
  if (log2n > 31 || (int)log2n > kzgx_ntt_max_log2(g_curve))
    throw std::invalid_argument(std::string(where) + ": the domain exceeds the curve's power-of-two domain");
  const size_t bb = (size_t)32 << log2n;
  if (blobs.size() % bb) throw std::invalid_argument(std::string(where) + ": not a whole number of blobs");
  return blobs.size() / bb;
}
}  // namespace

std::pair<std::vector<uint8_t>, std::vector<uint8_t>> trusted_setup::create_blob_proofs(
    const std::vector<uint8_t>& blobs, unsigned log2n, bool bit_reversed) {
  const size_t m = blob_count(blobs, log2n, "create_blob_proofs");
  std::vector<uint8_t> commits(48 * m), proofs(48 * m);
  const int flags = KZGX_BLOB_BYTES | (bit_reversed ? KZGX_NTT_BITREV : 0);
  check(kzgx_prove_blobs_batch(ctx, blobs.data(), log2n, m, flags, commits.data(), proofs.data(), nullptr, nullptr),
        "kzgx_prove_blobs_batch");
  return {std::move(commits), std::move(proofs)};
}

bool trusted_setup::verify_blob_proofs(const std::vector<uint8_t>& blobs, const std::vector<uint8_t>& commits,
                                       const std::vector<uint8_t>& proofs, unsigned log2n, bool bit_reversed,
                                       bool check_subgroup) {
  const size_t m = blob_count(blobs, log2n, "verify_blob_proofs");
  if (commits.size() != 48 * m || proofs.size() != 48 * m)
    throw std::invalid_argument("verify_blob_proofs: size mismatch");
  const int flags = KZGX_BLOB_BYTES | (bit_reversed ? KZGX_NTT_BITREV : 0);
  int ok = 0;
  check(kzgx_verify_blobs_batch(ctx, blobs.data(), log2n, m, flags, commits.data(), proofs.data(), nullptr,
                                check_subgroup ? 1 : 0, &ok),
        "kzgx_verify_blobs_batch");
  return ok != 0;
}

std::vector<bool> trusted_setup::verify_blob_proofs_each(const std::vector<uint8_t>& blobs,
                                                         const std::vector<uint8_t>& commits,
                                                         const std::vector<uint8_t>& proofs, unsigned log2n,
                                                         bool bit_reversed, bool check_subgroup) {
  const size_t m = blob_count(blobs, log2n, "verify_blob_proofs_each");
  if (commits.size() != 48 * m || proofs.size() != 48 * m)
    throw std::invalid_argument("verify_blob_proofs_each: size mismatch");
  const int flags = KZGX_BLOB_BYTES | (bit_reversed ? KZGX_NTT_BITREV : 0);
  std::vector<int> oks(m ? m : 1, 0);
  check(kzgx_verify_blobs_each(ctx, blobs.data(), log2n, m, flags, commits.data(), proofs.data(),
                               check_subgroup ? 1 : 0, oks.data()),
        "kzgx_verify_blobs_each");
  std::vector<bool> res;
  for (size_t k = 0; k < m; k++) res.push_back(oks[k] != 0);
  return res;
}

G1 trusted_setup::linear_combination(const std::vector<G1>& points, const std::vector<Fr>& scalars) {
  const size_t m = points.size();
  if (scalars.size() != m) throw std::invalid_argument("linear_combination: size mismatch");
  const int nl = base_limbs();
  std::vector<uint64_t> xy(2 * nl * m + 1, 0), s(4 * m + 1), out(2 * nl);
  std::vector<int> inf(m + 1);
  for (size_t k = 0; k < m; k++) {
    for (int i = 0; i < nl; i++) {
      xy[2 * nl * k + i] = points[k].x[i];
      xy[2 * nl * k + nl + i] = points[k].y[i];
    }
    inf[k] = points[k].inf;
    std::memcpy(&s[4 * k], scalars[k].v.data(), 32);
  }
  int oi = 1;
  check(kzgx_msm_g1_points(ctx, xy.data(), inf.data(), s.data(), m, out.data(), &oi), "kzgx_msm_g1_points");
  return to_g1(out.data(), oi != 0);
}

namespace {
// groups -> the C ABI's flat claim list: index per claim, group_start, one point per group
struct batch_claims {
  std::vector<uint32_t> index, start;
  std::vector<uint64_t> zs, gammas;
};

batch_claims flatten_groups(const std::vector<batch_opening>& groups, const std::vector<Fr>& gammas, size_t n_index,
                            const char* who) {
  if (gammas.size() != groups.size()) throw std::invalid_argument(std::string(who) + ": one gamma per group");
  batch_claims c;
  c.start.push_back(0);
  for (size_t g = 0; g < groups.size(); g++) {
    for (uint32_t j : groups[g].polys) {
      if (j >= n_index) throw std::invalid_argument(std::string(who) + ": index out of range");
      c.index.push_back(j);
    }
    c.start.push_back((uint32_t)c.index.size());
    c.zs.insert(c.zs.end(), groups[g].point.v.begin(), groups[g].point.v.end());
    c.gammas.insert(c.gammas.end(), gammas[g].v.begin(), gammas[g].v.end());
  }
  return c;
}
}  // namespace

std::vector<proof> trusted_setup::create_batch_proofs(const std::vector<kzg::poly>& polys,
                                                      const std::vector<batch_opening>& groups,
                                                      const std::vector<Fr>& gammas,
                                                      std::vector<std::vector<Fr>>* values_out) {
  batch_claims cl = flatten_groups(groups, gammas, polys.size(), "create_batch_proofs");
  std::vector<proof> res;
  if (values_out) values_out->clear();
  if (groups.empty()) return res;
  size_t m = 1;  // zero-padded to a common length (the zero polynomial: one zero coefficient)
  for (auto& p : polys) m = std::max(m, p.get_poly().size());
  if (m - 1 > n) throw std::invalid_argument("polynomial degree be at most one less than the setup size (num_coeffs)");
  std::vector<uint64_t> s(4 * m * std::max<size_t>(polys.size(), 1), 0);
  for (size_t b = 0; b < polys.size(); b++) {
    auto f = flat(polys[b].get_poly());
    if (!f.empty()) std::memcpy(&s[4 * m * b], f.data(), f.size() * 8);
  }
  const int nl = base_limbs();
  const size_t count = cl.index.size(), ng = groups.size();
  std::vector<uint64_t> out(2 * nl * ng), y(4 * count + 4);
  std::vector<int> inf(ng);
  cl.index.push_back(0);  // never NULL
  check(kzgx_prove_multi_batch(ctx, s.data(), m, m, polys.size(), cl.index.data(), cl.start.data(), ng, cl.zs.data(),
                               cl.gammas.data(), count, KZGX_MULTI_WEIGHT_POWERS, out.data(), inf.data(),
                               values_out ? y.data() : nullptr, nullptr),
        "kzgx_prove_multi_batch");
  for (size_t g = 0; g < ng; g++) res.push_back(proof(to_g1(&out[2 * nl * g], inf[g])));
  if (values_out)
    for (size_t g = 0; g < ng; g++) {
      std::vector<Fr> v(cl.start[g + 1] - cl.start[g]);
      for (size_t j = 0; j < v.size(); j++) std::memcpy(v[j].v.data(), &y[4 * (cl.start[g] + j)], 32);
      values_out->push_back(std::move(v));
    }
  return res;
}

bool trusted_setup::verify_batch_proofs(std::vector<commit>& commits, const std::vector<batch_opening>& groups,
                                        const std::vector<Fr>& gammas, const std::vector<std::vector<Fr>>& values,
                                        std::vector<proof>& proofs) {
  return batch_verified(commits, groups, gammas, values, proofs, false, false);
}

bool trusted_setup::verify_batch_proofs(std::vector<commit>& commits, const std::vector<batch_opening>& groups,
                                        const std::vector<Fr>& gammas, const std::vector<std::vector<Fr>>& values,
                                        std::vector<proof>& proofs, bool check_subgroup) {
  return batch_verified(commits, groups, gammas, values, proofs, true, check_subgroup);
}

bool trusted_setup::batch_verified(std::vector<commit>& commits, const std::vector<batch_opening>& groups,
                                   const std::vector<Fr>& gammas, const std::vector<std::vector<Fr>>& values,
                                   std::vector<proof>& proofs, bool checked, bool check_subgroup) {
  batch_claims cl = flatten_groups(groups, gammas, commits.size(), "verify_batch_proofs");
  const size_t ng = groups.size(), nc = commits.size(), count = cl.index.size();
  if (proofs.size() != ng || values.size() != ng) throw std::invalid_argument("verify_batch_proofs: size mismatch");
  std::vector<uint64_t> y;
  for (size_t g = 0; g < ng; g++) {
    if (values[g].size() != groups[g].polys.size())
      throw std::invalid_argument("verify_batch_proofs: one value per opened commitment");
    for (auto& v : values[g]) y.insert(y.end(), v.v.begin(), v.v.end());
  }
  if (ng == 0) return true;
  const int nl = base_limbs();
  std::vector<uint64_t> c(2 * nl * nc + 1, 0), p(2 * nl * ng, 0);
  std::vector<int> ci(nc + 1), pi(ng);
  for (size_t k = 0; k < nc; k++) {
    const G1& cg = commits[k].get_curve_point();
    for (int i = 0; i < nl; i++) {
      c[2 * nl * k + i] = cg.x[i];
      c[2 * nl * k + nl + i] = cg.y[i];
    }
    ci[k] = cg.inf;
  }
  for (size_t g = 0; g < ng; g++) {
    const G1& pg = proofs[g].get_curve_point();
    for (int i = 0; i < nl; i++) {
      p[2 * nl * g + i] = pg.x[i];
      p[2 * nl * g + nl + i] = pg.y[i];
    }
    pi[g] = pg.inf;
  }
  cl.index.push_back(0);  // never NULL
  y.resize(y.size() + 4);
  int ok = 0;
  if (checked)
    check(kzgx_verify_multi_batch_checked(ctx, c.data(), ci.data(), nc, cl.index.data(), cl.start.data(), ng,
                                          cl.zs.data(), y.data(), cl.gammas.data(), p.data(), pi.data(), nullptr,
                                          count, KZGX_MULTI_WEIGHT_POWERS, check_subgroup ? 1 : 0, &ok),
          "kzgx_verify_multi_batch_checked");
  else
    check(kzgx_verify_multi_batch(ctx, c.data(), ci.data(), nc, cl.index.data(), cl.start.data(), ng, cl.zs.data(),
                                  y.data(), cl.gammas.data(), p.data(), pi.data(), nullptr, count,
                                  KZGX_MULTI_WEIGHT_POWERS, &ok),
          "kzgx_verify_multi_batch");
  return ok != 0;
}

namespace {
// sets -> the C ABI's flat table: point indices and claim indices set by set, with their start arrays
struct shplonk_table {
  std::vector<uint32_t> sps, sp, cs, index;
  std::vector<uint64_t> t;
  size_t n_values = 0;
};

shplonk_table flatten_sets(const std::vector<Fr>& points, const std::vector<shplonk_set>& sets, size_t n_index,
                           const char* who) {
  if (sets.empty() || points.empty()) throw std::invalid_argument(std::string(who) + ": no sets or no points");
  shplonk_table c;
  c.sps.push_back(0);
  c.cs.push_back(0);
  for (auto& s : sets) {
    if (s.points.empty() || s.points.size() > KZGX_SHPLONK_SET_MAX)
      throw std::invalid_argument(std::string(who) + ": 1 .. KZGX_SHPLONK_SET_MAX points per set");
    for (size_t a = 0; a < s.points.size(); a++) {
      if (s.points[a] >= points.size()) throw std::invalid_argument(std::string(who) + ": point index out of range");
      for (size_t b = 0; b < a; b++)
        if (s.points[a] == s.points[b]) throw std::invalid_argument(std::string(who) + ": an index twice in one set");
      c.sp.push_back(s.points[a]);
    }
    for (uint32_t j : s.polys) {
      if (j >= n_index) throw std::invalid_argument(std::string(who) + ": index out of range");
      c.index.push_back(j);
    }
    c.sps.push_back((uint32_t)c.sp.size());
    c.cs.push_back((uint32_t)c.index.size());
    c.n_values += s.points.size() * s.polys.size();
  }
  for (auto& p : points) c.t.insert(c.t.end(), p.v.begin(), p.v.end());
  c.index.push_back(0);  // never NULL
  return c;
}
}  // namespace

shplonk_proof trusted_setup::create_shplonk_proof(const std::vector<kzg::poly>& polys, const std::vector<Fr>& points,
                                                  const std::vector<shplonk_set>& sets, const Fr& gamma,
                                                  const std::function<Fr(const proof&)>& challenge,
                                                  std::vector<std::vector<Fr>>* values_out) {
  shplonk_table tb = flatten_sets(points, sets, polys.size(), "create_shplonk_proof");
  if (!challenge) throw std::invalid_argument("create_shplonk_proof: no challenge function");
  size_t m = 1;  // zero-padded to a common length (the zero polynomial: one zero coefficient)
  for (auto& p : polys) m = std::max(m, p.get_poly().size());
  if (m - 1 > n) throw std::invalid_argument("polynomial degree be at most one less than the setup size (num_coeffs)");
  std::vector<uint64_t> s(4 * m * std::max<size_t>(polys.size(), 1), 0);
  for (size_t b = 0; b < polys.size(); b++) {
    auto f = flat(polys[b].get_poly());
    if (!f.empty()) std::memcpy(&s[4 * m * b], f.data(), f.size() * 8);
  }
  const int nl = base_limbs();
  const size_t count = tb.index.size() - 1;
  std::vector<uint64_t> out(2 * nl), h(4 * m), y(4 * tb.n_values + 4);
  int inf = 0;
  check(kzgx_shplonk_commit(ctx, s.data(), m, m, polys.size(), tb.t.data(), points.size(), tb.sps.data(),
                            tb.sp.data(), tb.sp.size(), tb.cs.data(), tb.index.data(), sets.size(), gamma.v.data(),
                            count, tb.n_values, KZGX_SHPLONK_WEIGHT_POWERS, out.data(), &inf, h.data(),
                            values_out ? y.data() : nullptr),
        "kzgx_shplonk_commit");
  shplonk_proof res{proof(to_g1(out.data(), inf)), proof(to_g1(out.data(), 1))};
  const Fr z = challenge(res.W);
  check(kzgx_shplonk_open(ctx, s.data(), m, m, polys.size(), tb.t.data(), points.size(), tb.sps.data(), tb.sp.data(),
                          tb.sp.size(), tb.cs.data(), tb.index.data(), sets.size(), gamma.v.data(), count,
                          KZGX_SHPLONK_WEIGHT_POWERS, h.data(), z.v.data(), out.data(), &inf, nullptr),
        "kzgx_shplonk_open");
  res.Wp = proof(to_g1(out.data(), inf));
  if (values_out) {
    values_out->clear();
    size_t v = 0;
    for (auto& st : sets) {
      std::vector<Fr> vals(st.points.size() * st.polys.size());
      for (auto& f : vals) {
        std::memcpy(f.v.data(), &y[4 * v], 32);
        v++;
      }
      values_out->push_back(std::move(vals));
    }
  }
  return res;
}

bool trusted_setup::verify_shplonk_proof(std::vector<commit>& commits, const std::vector<Fr>& points,
                                         const std::vector<shplonk_set>& sets, const Fr& gamma,
                                         const std::vector<std::vector<Fr>>& values, const Fr& z,
                                         shplonk_proof& proof) {
  return shplonk_verified(commits, points, sets, gamma, values, z, proof, false, false);
}

bool trusted_setup::verify_shplonk_proof(std::vector<commit>& commits, const std::vector<Fr>& points,
                                         const std::vector<shplonk_set>& sets, const Fr& gamma,
                                         const std::vector<std::vector<Fr>>& values, const Fr& z,
                                         shplonk_proof& proof, bool check_subgroup) {
  return shplonk_verified(commits, points, sets, gamma, values, z, proof, true, check_subgroup);
}

bool trusted_setup::shplonk_verified(std::vector<commit>& commits, const std::vector<Fr>& points,
                                     const std::vector<shplonk_set>& sets, const Fr& gamma,
                                     const std::vector<std::vector<Fr>>& values, const Fr& z, shplonk_proof& pr,
                                     bool checked, bool check_subgroup) {
  shplonk_table tb = flatten_sets(points, sets, commits.size(), "verify_shplonk_proof");
  if (values.size() != sets.size()) throw std::invalid_argument("verify_shplonk_proof: size mismatch");
  std::vector<uint64_t> y;
  for (size_t s = 0; s < sets.size(); s++) {
    if (values[s].size() != sets[s].points.size() * sets[s].polys.size())
      throw std::invalid_argument("verify_shplonk_proof: one value per opened commitment and point");
    for (auto& v : values[s]) y.insert(y.end(), v.v.begin(), v.v.end());
  }
  y.resize(y.size() + 4);
  const int nl = base_limbs();
  const size_t nc = commits.size(), count = tb.index.size() - 1;
  std::vector<uint64_t> c(2 * nl * nc + 1, 0), p(4 * nl, 0);
  std::vector<int> ci(nc + 1), pi(2);
  for (size_t k = 0; k < nc; k++) {
    const G1& cg = commits[k].get_curve_point();
    for (int i = 0; i < nl; i++) {
      c[2 * nl * k + i] = cg.x[i];
      c[2 * nl * k + nl + i] = cg.y[i];
    }
    ci[k] = cg.inf;
  }
  proof* both[2] = {&pr.W, &pr.Wp};
  for (int g = 0; g < 2; g++) {
    const G1& pg = both[g]->get_curve_point();
    for (int i = 0; i < nl; i++) {
      p[2 * nl * g + i] = pg.x[i];
      p[2 * nl * g + nl + i] = pg.y[i];
    }
    pi[g] = pg.inf;
  }
  int ok = 0;
  if (checked)
    check(kzgx_shplonk_verify_checked(ctx, c.data(), ci.data(), nc, tb.index.data(), tb.t.data(), points.size(),
                                      tb.sps.data(), tb.sp.data(), tb.sp.size(), tb.cs.data(), sets.size(), y.data(),
                                      tb.n_values, gamma.v.data(), count, z.v.data(), p.data(), pi.data(),
                                      KZGX_SHPLONK_WEIGHT_POWERS, check_subgroup ? 1 : 0, &ok),
          "kzgx_shplonk_verify_checked");
  else
    check(kzgx_shplonk_verify(ctx, c.data(), ci.data(), nc, tb.index.data(), tb.t.data(), points.size(),
                              tb.sps.data(), tb.sp.data(), tb.sp.size(), tb.cs.data(), sets.size(), y.data(),
                              tb.n_values, gamma.v.data(), count, z.v.data(), p.data(), pi.data(),
                              KZGX_SHPLONK_WEIGHT_POWERS, &ok),
          "kzgx_shplonk_verify");
  return ok != 0;
}

std::vector<G1> trusted_setup::g1_points() const {
  const int nl = base_limbs();
  std::vector<uint64_t> xy(2 * nl * n);
  check(kzgx_get_srs_g1(ctx, xy.data(), n), "kzgx_get_srs_g1");
  std::vector<G1> res;
  for (size_t i = 0; i < n; i++) {
    bool z = true;
    for (int k = 0; k < 2 * nl; k++) z &= xy[2 * nl * i + k] == 0;
    res.push_back(to_g1(&xy[2 * nl * i], z));
  }
  return res;
}

void trusted_setup::precompute(int window_bits, size_t points) {
  check(kzgx_set_fixed_base(ctx, window_bits, window_bits ? (points ? std::min(points, n) : n) : 0),
        "kzgx_set_fixed_base");
}

void trusted_setup::default_table(int window_bits, size_t points) {
  check(kzgx_set_default_table(ctx, window_bits, window_bits ? points : 0), "kzgx_set_default_table");
}

int trusted_setup::precompute_budget(size_t budget_bytes, size_t points) {
  int c = 0;
  check(kzgx_set_fixed_base_budget(ctx, budget_bytes, points ? std::min(points, n) : n, &c),
        "kzgx_set_fixed_base_budget");
  return c;
}

std::vector<G2> trusted_setup::g2_points() const {
  const int nl = base_limbs();
  const size_t n2 = kzgx_srs_g2_size(ctx);
  std::vector<uint64_t> xy(4 * nl * n2);
  if (n2) check(kzgx_get_srs_g2(ctx, xy.data(), n2), "kzgx_get_srs_g2");
  std::vector<G2> res;
  for (size_t i = 0; i < n2; i++) {
    bool z = true;
    for (int k = 0; k < 4 * nl; k++) z &= xy[4 * nl * i + k] == 0;
    res.push_back(to_g2(&xy[4 * nl * i], z));
  }
  return res;
}

}  // namespace kzg
