// plugin_mi355x.cc — libec_mi355x.so: the MI355X EC plugin behind the
// reference's plugin contract. Pattern mirrors the reference's plugin shims
// (src/erasure-code/jerasure/ErasureCodePluginJerasure.cc:35-90 factory
// dispatch + entry points; src/erasure-code/isa glue marshalling,
// ErasureCodeIsa.cc:118-243). All byte/stripe compute goes through the
// C-ABI into the gfx950 kernels (include/ec_mi355x.h); there is no CPU
// fallback — init() fails with -ENODEV when no GPU is visible.
#include <cerrno>
#include <cstring>
#include <iostream>
#include <memory>
#include <ostream>
#include <sstream>

#include "../../include/ec_mi355x.h"
#include "erasure_code_plugin.h"

using namespace ecx;

namespace {

int technique_id(const std::string &t) {
  if (t == "reed_sol_van") return ECX_T_RS_VAN_ISA;
  if (t == "cauchy") return ECX_T_CAUCHY_ISA;
  if (t == "jerasure_reed_sol_van") return ECX_T_RS_VAN_JERASURE;
  if (t == "cauchy_orig") return ECX_T_CAUCHY_ORIG_JERASURE;
  if (t == "cauchy_good") return ECX_T_CAUCHY_GOOD_JERASURE;
  // jerasure reed_sol_r6_op (RAID6, m==2): its reed_sol_r6_coding_matrix
  // is row0 = all ones, row1 = [2^j] — byte-identical to the isa RS-van
  // construction at m=2 (gf_gen_rs_matrix rows k, k+1)
  if (t == "reed_sol_r6_op") return ECX_T_RS_VAN_ISA;
  return -1;
}

class ErasureCodeMi355x final : public ErasureCode {
  ecx_ctx *ctx_ = nullptr;
  int k_ = 0, m_ = 0, w_ = 8, device_ = 0, streams_ = 2, packetsize_ = 2048;
  std::string technique_;
  bool is_bitmatrix() const {
    int t = technique_id(technique_);
    return t == ECX_T_CAUCHY_ORIG_JERASURE || t == ECX_T_CAUCHY_GOOD_JERASURE;
  }

 public:
  explicit ErasureCodeMi355x(std::string technique)
      : technique_(std::move(technique)) {}
  ~ErasureCodeMi355x() override {
    if (ctx_) ecx_destroy(ctx_);
  }

  unsigned int get_chunk_count() const override { return k_ + m_; }
  unsigned int get_data_chunk_count() const override { return k_; }
  size_t get_minimum_granularity() override { return 16; }

  plugin_flags get_supported_optimizations() const override {
    // mirror the upstream plugin that owns each technique, flag for flag:
    // isa techniques (ErasureCodeIsa.h:66-79) claim OPTIMIZED always and
    // CRC for reed_sol_van (cauchy only at m=1); jerasure techniques
    // (ErasureCodeJerasure.h:52-63) claim OPTIMIZED only for reed_sol_van
    // and CRC for everything except reed_sol_van and cauchy_orig. The CRC
    // flag is a capability declaration the OSD's scrub consumes — there
    // is no plugin-side CRC method to implement. Parity-delta is claimed
    // for every technique, as upstream does (matrix deltas via
    // matrix_apply_delta, bitmatrix deltas via schedule_apply_delta —
    // both implemented here; delta == re-encode is conformance-tested).
    plugin_flags f = FLAG_EC_PLUGIN_PARTIAL_READ_OPTIMIZATION |
                     FLAG_EC_PLUGIN_PARTIAL_WRITE_OPTIMIZATION |
                     FLAG_EC_PLUGIN_ZERO_INPUT_ZERO_OUTPUT_OPTIMIZATION |
                     FLAG_EC_PLUGIN_PARITY_DELTA_OPTIMIZATION |
                     FLAG_EC_PLUGIN_DIRECT_READS;
    if (technique_ == "reed_sol_van" || technique_ == "cauchy") {
      // isa-matrix techniques
      f |= FLAG_EC_PLUGIN_OPTIMIZED_SUPPORTED;
      if (technique_ == "reed_sol_van" ||
          (technique_ == "cauchy" && m_ == 1))
        f |= FLAG_EC_PLUGIN_CRC_ENCODE_DECODE_SUPPORT;
    } else if (technique_ == "jerasure_reed_sol_van") {
      f |= FLAG_EC_PLUGIN_OPTIMIZED_SUPPORTED;  // jerasure reed_sol_van
    } else if (technique_ != "cauchy_orig") {
      // jerasure family: CRC for everything but reed_sol_van/cauchy_orig
      // (ErasureCodeJerasure.h:57-62) — cauchy_good and reed_sol_r6_op
      f |= FLAG_EC_PLUGIN_CRC_ENCODE_DECODE_SUPPORT;
    }
    return f;
  }

  int parse(ErasureCodeProfile &profile, std::ostream *ss) {
    int err = ErasureCode::parse(profile, ss);
    err |= to_int("k", profile, &k_, "8", ss);
    err |= to_int("m", profile, &m_, "3", ss);
    err |= to_int("w", profile, &w_, "8", ss);
    err |= to_int("mi355x-device", profile, &device_, "0", ss);
    err |= to_int("mi355x-streams", profile, &streams_, "2", ss);
    if (is_bitmatrix())
      err |= to_int("packetsize", profile, &packetsize_, "2048", ss);
    err |= sanity_check_k_m(k_, m_, ss);
    // w=16 is supported for the jerasure RS-van technique (GF(2^16)
    // matrix, ErasureCodeJerasure.cc:421 accepts w in {8,16,32}; w=32 is
    // not implemented here)
    if (!(w_ == 8 ||
          (w_ == 16 && technique_ == "jerasure_reed_sol_van"))) {
      if (ss)
        *ss << "mi355x: w=" << w_
            << " must be 8 (or 16 with jerasure_reed_sol_van)\n";
      err = -EINVAL;
    }
    if (technique_id(technique_) < 0) {
      if (ss) *ss << "mi355x: unknown technique " << technique_ << "\n";
      err = -EINVAL;
    }
    if (technique_ == "cauchy_good" && m_ == 2) {
      // jerasure's m==2 cauchy_good reads precomputed cbest tables that
      // cannot be faithfully restated here; refuse rather than silently
      // diverge from the reference's parity bytes
      if (ss)
        *ss << "cauchy_good: m=2 uses jerasure's cbest tables "
               "(unsourceable here) — use cauchy_orig or m!=2\n";
      err = -EINVAL;
    }
    if (technique_ == "reed_sol_r6_op" && m_ != 2) {
      // ErasureCodeJerasureReedSolomonRAID6::parse (:473-488)
      if (ss) *ss << "reed_sol_r6_op: m=" << m_ << " must be 2 for RAID6\n";
      err = -EINVAL;
    }
    profile["technique"] = technique_;
    return err;
  }

  int init(ErasureCodeProfile &profile, std::ostream *ss) override {
    int err = parse(profile, ss);
    if (err) return err;
    int tid = technique_id(technique_);
    if (w_ == 16 && technique_ == "jerasure_reed_sol_van")
      tid = ECX_T_RS_VAN_JERASURE_W16;
    int r = ecx_create2(k_, m_, tid, w_, packetsize_, device_, streams_,
                        &ctx_);
    if (r != ECX_OK) {
      if (ss)
        *ss << "mi355x: ecx_create failed (" << r
            << (r == ECX_ERR_NO_GPU ? ": no GPU — this plugin has no CPU "
                                      "fallback"
                                    : "")
            << ")\n";
      return r;
    }
    return ErasureCode::init(profile, ss);
  }

  unsigned int get_chunk_size(unsigned int stripe_width) const override {
    return ecx_chunk_size(ctx_, stripe_width);
  }

  int encode_chunks(const shard_id_map<buffer> &in,
                    shard_id_map<buffer> &out) override {
    // marshalling mirror of ErasureCodeIsa.cc:118-165: absent shards are
    // zeros (NULL pointer convention of the C-ABI); sizes must agree
    size_t size = 0;
    const uint8_t *data[64] = {};
    uint8_t *parity[64] = {};
    for (auto &&[shard, b] : in) {
      if ((int)shard >= k_) return -EINVAL;
      if (!size) size = b.length();
      else if (size != b.length()) return -EINVAL;
      data[(int)shard] = b.c_str();
    }
    for (auto &&[shard, b] : out) {
      if (!size) size = b.length();
      else if (size != b.length()) return -EINVAL;
      if ((int)shard < k_) {
        // a data-position buffer arriving via the out map is a SOURCE —
        // the LRC local-layer pattern feeds upper-layer parity back in as
        // data this way (ErasureCodeLrc.cc:985-991 + isa marshalling
        // ErasureCodeIsa.cc:134-141 treat in/out symmetrically)
        data[(int)shard] = b.c_str();
      } else {
        parity[(int)shard - k_] = b.c_str();
      }
    }
    if (!size) return 0;
    return ecx_encode_chunks_host(ctx_, data, parity, size);
  }

  int decode_chunks(const shard_id_set &want_to_read,
                    shard_id_map<buffer> &in,
                    shard_id_map<buffer> &out) override {
    (void)want_to_read;  // all erasures in `out` are reconstructed
    // all in/out buffer lengths must agree (mirror of the encode_chunks
    // checks; the reference asserts equal blocksize per call,
    // ErasureCodeJerasure.cc:226-246) — mismatched lengths would reach
    // ecx_decode_chunks_host, which memcpys `size` bytes per chunk
    size_t size = 0;
    uint8_t *chunks[64] = {};
    uint64_t present = 0;
    std::vector<buffer> temps;
    for (auto &&[shard, b] : in) {
      if (!size) size = b.length();
      else if (size != b.length()) return -EINVAL;
      chunks[(int)shard] = b.c_str();
      present |= 1ull << (int)shard;
    }
    for (auto &&[shard, b] : out) {
      if (!size) size = b.length();
      else if (size != b.length()) return -EINVAL;
      chunks[(int)shard] = b.c_str();
      present &= ~(1ull << (int)shard);
    }
    if (!size) return 0;
    // chunks in neither map are erasures reconstructed into scratch and
    // discarded (the reference invents such buffers,
    // ErasureCodeJerasure.cc:230-240)
    for (int i = 0; i < k_ + m_; i++) {
      if (!chunks[i] && !(present & (1ull << i))) {
        temps.push_back(buffer::create_aligned(size));
        chunks[i] = temps.back().c_str();
      }
    }
    return ecx_decode_chunks_host(ctx_, chunks, present, size);
  }

  void encode_delta(const buffer &old_data, const buffer &new_data,
                    buffer *delta_maybe_in_place) override {
    int r = ecx_encode_delta_host(ctx_, old_data.c_str(), new_data.c_str(),
                                  delta_maybe_in_place->c_str(),
                                  delta_maybe_in_place->length());
    // void, as in the reference: a refusal leaves the delta unwritten, so
    // at least say so
    if (r != ECX_OK)
      std::cerr << "mi355x: encode_delta refused (" << r << ")\n";
  }

  void apply_delta(const shard_id_map<buffer> &in,
                   shard_id_map<buffer> &out) override {
    // the pairs of isa apply_delta's loop (ErasureCodeIsa.cc:333-366), same
    // filters, collected into ONE staged call: every delta and parity
    // crosses PCIe once. Bitmatrix techniques route to the schedule-delta
    // kernel inside it (schedule_apply_delta semantics)
    std::vector<const uint8_t *> deltas;
    std::vector<uint8_t *> parities;
    std::vector<int> datashards, codingshards;
    size_t size = 0;
    for (auto &&[datashard, databuf] : in) {
      if ((int)datashard >= k_) continue;
      deltas.push_back(databuf.c_str());
      datashards.push_back((int)datashard);
    }
    for (auto &&[codingshard, codingbuf] : out) {
      if ((int)codingshard < k_) continue;
      parities.push_back(const_cast<uint8_t *>(codingbuf.c_str()));
      codingshards.push_back((int)codingshard);
      size = codingbuf.length();
    }
    if (deltas.empty() || parities.empty()) return;
    int r = ecx_apply_deltas_host(ctx_, deltas.data(), datashards.data(),
                                  (int)deltas.size(), parities.data(),
                                  codingshards.data(), (int)parities.size(),
                                  size);
    if (r != ECX_OK)
      std::cerr << "mi355x: apply_delta refused (" << r
                << "), parity left unchanged\n";
  }
};

class ErasureCodePluginMi355x final : public ErasureCodePlugin {
 public:
  int factory(const std::string &, ErasureCodeProfile &profile,
              ErasureCodeInterfaceRef *erasure_code,
              std::ostream *ss) override {
    std::string technique = "reed_sol_van";
    if (auto it = profile.find("technique"); it != profile.end())
      technique = it->second;
    auto interface = std::make_shared<ErasureCodeMi355x>(technique);
    int r = interface->init(profile, ss);
    if (r) return r;
    *erasure_code = interface;
    return 0;
  }
};

}  // namespace

// plugin C entry points (pattern: ErasureCodePluginJerasure.cc:74-90)
extern "C" {

const char *__erasure_code_version() { return ECX_HARNESS_VERSION; }

int __erasure_code_init(const char *plugin_name, const char *) {
  auto &instance = ErasureCodePluginRegistry::instance();
  auto plugin = std::make_unique<ErasureCodePluginMi355x>();
  int r = instance.add(plugin_name, plugin.get());
  if (r == 0) plugin.release();
  return r;
}
}
