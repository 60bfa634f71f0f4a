// ec_plugin_diff.cc — differential test of two EC plugins at the
// ErasureCodeInterface boundary, the boundary Ceph itself calls.
//
// Both plugins (REF and DUT) are created through the registry factory, fed
// the same bytes (splitmix64 from --seed) and compared method by method:
// return code, key set and bytes. The first difference is printed as one
// "DIFF step=... width=... shard=... offset=... ref=0x.. dut=0x.." line and
// the tool exits 1. Without a difference it prints one "WIDTH w chunk=C"
// line per width, one "STEP name compared=N" (or "STEP name skipped=reason")
// line per step, then DIFF_OK.
//
// Every buffer handed to a plugin is a substr() view into a larger
// allocation filled with 0xA5, with at least 64 guard bytes on each side.
// After each call the guards must be intact and every buffer the call may
// not write (all inputs, outputs held back from the call) must be
// unchanged. Each width runs twice: views at offset 64, then at 64 + 16 so
// the plugin's staging copies see pointers that are not 64-byte aligned.
//
// Steps (see usage()): shape, minimum, encode, encode_want, encode_chunks,
// decode, decode_chunks, delta, repeat. `shape` always runs, --only or not:
// every other step relies on both sides agreeing on the geometry. The
// erasure patterns are short fixed lists (no random subsets), so a failure
// reproduces from the command line alone.
//
// decode_chunks is overridden by every plugin of this tree (it is pure in
// the base class), so no plugin skips that step. Its case (c), a present
// shard left out of `in`, is treated by every plugin here as one more
// erasure (a chunk in neither map is rebuilt into scratch): with the
// m-erasure pattern that makes m+1, so both sides must refuse alike.
//
// --delta-vs-reencode is for plugins without a CPU twin (shec): it runs the
// delta step only, on DUT alone, and checks the delta-updated parity against
// DUT's own encode_chunks of the new data.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "erasure_code.h"
#include "erasure_code_plugin.h"

using ecx::buffer;
using ecx::ErasureCodeInterface;
using ecx::ErasureCodeInterfaceRef;
using ecx::ErasureCodePluginRegistry;
using ecx::ErasureCodeProfile;
using ecx::shard_id_map;
using ecx::shard_id_set;
using ecx::shard_id_t;

namespace {

constexpr uint8_t POISON = 0xA5;
constexpr size_t GUARD = 64;
using Bytes = std::vector<uint8_t>;

const char *const STEPS[] = {"shape",         "minimum", "encode",
                             "encode_want",   "encode_chunks", "decode",
                             "decode_chunks", "delta",   "repeat"};

struct Diff {};  // thrown at the first difference; main() turns it into exit 1

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  Bytes bytes(size_t n) {
    Bytes b(n);
    for (size_t i = 0; i < n; i += 8) {
      uint64_t v = next();
      std::memcpy(&b[i], &v, std::min<size_t>(8, n - i));
    }
    return b;
  }
};

// where we are, for the DIFF line
std::string g_step;
unsigned g_width = 0;
size_t g_view_off = 0;

std::string where(const std::string &call) {
  std::ostringstream o;
  o << "DIFF step=" << g_step << " width=" << g_width
    << " view_offset=" << g_view_off << " call=" << call;
  return o.str();
}

[[noreturn]] void fail(const std::string &call, const std::string &what) {
  std::cout << where(call) << " " << what << std::endl;
  throw Diff{};
}

void cmp_bytes(const std::string &call, int shard, const Bytes &ref,
               const Bytes &dut, const char *ref_name = "ref",
               const char *dut_name = "dut") {
  if (ref.size() != dut.size()) {
    std::ostringstream o;
    o << "shard=" << shard << " length " << ref_name << "=" << ref.size()
      << " " << dut_name << "=" << dut.size();
    fail(call, o.str());
  }
  for (size_t i = 0; i < ref.size(); i++)
    if (ref[i] != dut[i]) {
      char line[128];
      std::snprintf(line, sizeof line,
                    "shard=%d offset=%zu %s=0x%02x %s=0x%02x", shard, i,
                    ref_name, ref[i], dut_name, dut[i]);
      fail(call, line);
    }
}

// A caller buffer: `view` sits inside `raw` with poison all round it.
struct GBuf {
  buffer raw, view;
  Bytes expect;  // what the view holds as long as nobody may write it
  static GBuf make(size_t len, const uint8_t *src) {
    GBuf g;
    g.raw = buffer::create_aligned(g_view_off + len + GUARD);
    std::memset(g.raw.c_str(), POISON, g.raw.length());
    g.view = g.raw.substr(g_view_off, len);
    if (src) std::memcpy(g.view.c_str(), src, len);
    g.expect.assign(g.view.c_str(), g.view.c_str() + len);
    return g;
  }
  static GBuf input(const Bytes &b) { return make(b.size(), b.data()); }
  static GBuf output(size_t len) { return make(len, nullptr); }
  Bytes bytes() const {
    return Bytes(view.c_str(), view.c_str() + view.length());
  }
  // guards intact; written=false: the view is unchanged as well
  void verify(const std::string &call, const std::string &side, int shard,
              bool written) const {
    const uint8_t *p = raw.c_str();
    const size_t lo = g_view_off, hi = g_view_off + view.length();
    for (size_t i = 0; i < raw.length(); i++) {
      if (i >= lo && i < hi) continue;
      if (p[i] != POISON) {
        std::ostringstream o;
        o << side << " wrote a guard byte: shard=" << shard << " at "
          << (long)i - (long)lo << " relative to the buffer";
        fail(call, o.str());
      }
    }
    if (!written && std::memcmp(view.c_str(), expect.data(), expect.size())) {
      size_t i = 0;
      while (view.c_str()[i] == expect[i]) i++;
      std::ostringstream o;
      o << side << " wrote a buffer the call must not write: shard=" << shard
        << " offset=" << i;
      fail(call, o.str());
    }
  }
};

struct Side {
  std::string name;  // "ref" / "dut"
  ErasureCodeInterfaceRef ec;
};

// one call's outcome on one side
struct Res {
  int rc = 0;
  std::set<int> keys;            // key set of the returned map
  std::map<int, Bytes> out;      // the bytes that are compared
};

struct Geometry {
  int n = 0, k = 0, m = 0;
  std::vector<int> data, parity;  // shard id of raw data i / raw parity j
  unsigned C = 0;
};

struct Options {
  std::string dir = ".", ref, dut;
  ErasureCodeProfile ref_profile, dut_profile;
  std::vector<unsigned> widths;
  uint64_t seed = 1;
  std::set<std::string> only;
  bool delta_vs_reencode = false;
};

int usage() {
  std::cerr
      << "usage: ec_plugin_diff -d DIR --ref PLUGIN --dut PLUGIN\n"
         "         [-P k=v ...] [--ref-P k=v ...] [--dut-P k=v ...]\n"
         "         -s WIDTH [-s WIDTH ...] [--seed N] [--only STEP,...]\n"
         "         [--delta-vs-reencode]\n"
         "steps: shape minimum encode encode_want encode_chunks decode\n"
         "       decode_chunks delta repeat\n";
  return 2;
}

std::map<std::string, long> g_compared;
std::map<unsigned, unsigned> g_chunk_of;  // width -> chunk size, for the report
std::map<std::string, std::string> g_skipped;

void compare(const std::string &call, const Res &ref, const Res &dut) {
  if (ref.rc != dut.rc) {
    std::ostringstream o;
    o << "return code ref=" << ref.rc << " dut=" << dut.rc;
    fail(call, o.str());
  }
  if (ref.keys != dut.keys) {
    std::ostringstream o;
    o << "key set ref={";
    for (int s : ref.keys) o << s << ",";
    o << "} dut={";
    for (int s : dut.keys) o << s << ",";
    o << "}";
    fail(call, o.str());
  }
  if (ref.rc == 0) {
    for (auto &[shard, b] : ref.out) {
      auto it = dut.out.find(shard);
      if (it == dut.out.end()) fail(call, "dut lacks shard " + std::to_string(shard));
      cmp_bytes(call, shard, b, it->second);
    }
  }
  g_compared[g_step]++;
}

std::string set_name(const std::set<int> &s) {
  std::string o = "{";
  for (int x : s) o += (o.size() > 1 ? "," : "") + std::to_string(x);
  return o + "}";
}

shard_id_set to_shard_set(const std::set<int> &s) {
  shard_id_set o;
  for (int x : s) o.insert(x);
  return o;
}

// ---- the calls, one side at a time ----------------------------------------

Res do_encode(Side &s, const Geometry &g, const std::set<int> &want,
              const Bytes &in_master, const std::string &call) {
  Res r;
  GBuf in = GBuf::input(in_master);
  shard_id_map<buffer> enc(g.n);
  r.rc = s.ec->encode(to_shard_set(want), in.view, &enc);
  in.verify(call, s.name, -1, false);
  if (r.rc) return r;
  for (auto &&[shard, b] : enc) {
    r.keys.insert((int)shard);
    r.out[(int)shard] = Bytes(b.c_str(), b.c_str() + b.length());
  }
  return r;
}

// encode_chunks with raw data indices `absent` left out, `via_out` passed
// through the out map (sources, must stay unchanged) and raw parity indices
// `parities` asked for
Res do_encode_chunks(Side &s, const Geometry &g, const std::vector<Bytes> &data,
                     const std::set<int> &absent, const std::set<int> &via_out,
                     const std::vector<int> &parities,
                     const std::string &call) {
  Res r;
  std::map<int, GBuf> src, par;
  shard_id_map<buffer> in(g.n), out(g.n);
  for (int i = 0; i < g.k; i++) {
    if (absent.count(i)) continue;
    src[i] = GBuf::input(data[i]);
    (via_out.count(i) ? out : in)[g.data[i]] = src[i].view;
  }
  for (int j : parities) {
    par[j] = GBuf::output(g.C);
    out[g.parity[j]] = par[j].view;
  }
  r.rc = s.ec->encode_chunks(in, out);
  for (auto &[i, b] : src) b.verify(call, s.name, g.data[i], false);
  for (auto &[j, b] : par) b.verify(call, s.name, g.parity[j], true);
  for (auto &[j, b] : par) {
    r.keys.insert(g.parity[j]);
    r.out[g.parity[j]] = b.bytes();
  }
  return r;
}

// decode() of `want` from the chunks of `held` that are not in `erased`
Res do_decode(Side &s, const Geometry &g, const std::vector<GBuf> &held,
              const std::set<int> &want, const std::set<int> &erased,
              const std::string &call) {
  Res r;
  shard_id_map<buffer> chunks(g.n), decoded(g.n);
  for (int i = 0; i < g.n; i++)
    if (!erased.count(i)) chunks[i] = held[i].view;
  r.rc = s.ec->decode(to_shard_set(want), chunks, &decoded, (int)g.C);
  for (int i = 0; i < g.n; i++) held[i].verify(call, s.name, i, false);
  if (r.rc) return r;
  for (auto &&[shard, b] : decoded) {
    r.keys.insert((int)shard);
    // an erased shard nobody asked for may be left unrecovered (lrc stops
    // at the first layer that satisfies the request): only wanted bytes
    if (want.count((int)shard))
      r.out[(int)shard] = Bytes(b.c_str(), b.c_str() + b.length());
  }
  return r;
}

// decode_chunks() called directly: `erased` minus `neither` go to `out`,
// everything else but `left_out` and `neither` goes to `in`
Res do_decode_chunks(Side &s, const Geometry &g, const std::vector<GBuf> &held,
                     const std::set<int> &erased, const std::set<int> &neither,
                     const std::set<int> &left_out, const std::string &call) {
  Res r;
  std::map<int, GBuf> outs;
  std::set<int> want;
  shard_id_map<buffer> in(g.n), out(g.n);
  for (int i = 0; i < g.n; i++) {
    if (neither.count(i) || left_out.count(i)) continue;
    if (erased.count(i)) {
      outs[i] = GBuf::output(g.C);
      out[i] = outs[i].view;
      want.insert(i);
    } else {
      in[i] = held[i].view;
    }
  }
  r.rc = s.ec->decode_chunks(to_shard_set(want), in, out);
  for (int i = 0; i < g.n; i++) held[i].verify(call, s.name, i, false);
  for (auto &[i, b] : outs) b.verify(call, s.name, i, true);
  for (auto &[i, b] : outs) {
    r.keys.insert(i);
    r.out[i] = b.bytes();
  }
  return r;
}

struct DeltaRes {
  Res deltas, all, last_only, with_parity_entry;
};

// overwrite raw data indices `set` of `data` with `fresh`; parity0 is the
// parity of `data` by raw parity index
DeltaRes do_delta(Side &s, const Geometry &g, const std::vector<Bytes> &data,
                  const std::map<int, Bytes> &fresh,
                  const std::vector<Bytes> &parity0, const Bytes &junk,
                  const std::string &call) {
  DeltaRes r;
  for (auto &[i, nb] : fresh) {
    GBuf o = GBuf::input(data[i]), nw = GBuf::input(nb);
    GBuf d = GBuf::output(g.C);
    s.ec->encode_delta(o.view, nw.view, &d.view);
    o.verify(call + " encode_delta", s.name, g.data[i], false);
    nw.verify(call + " encode_delta", s.name, g.data[i], false);
    d.verify(call + " encode_delta", s.name, g.data[i], true);
    r.deltas.keys.insert(g.data[i]);
    r.deltas.out[g.data[i]] = d.bytes();
  }
  // 0: every parity in out; 1: the last parity only, the others held back
  // and unchanged; 2: as 0 with a parity-id entry in `in`, which is ignored
  Res *const results[3] = {&r.all, &r.last_only, &r.with_parity_entry};
  const char *const names[3] = {" apply_delta(a)", " apply_delta(b)",
                                " apply_delta(c)"};
  for (int v = 0; v < 3; v++) {
    const std::string c = call + names[v];
    std::map<int, GBuf> ins;
    std::vector<GBuf> pars;
    shard_id_map<buffer> in(g.n), out(g.n);
    for (auto &[shard, bytes] : r.deltas.out) {
      ins[shard] = GBuf::input(bytes);
      in[shard] = ins[shard].view;
    }
    if (v == 2) {
      ins[g.parity[0]] = GBuf::input(junk);
      in[g.parity[0]] = ins[g.parity[0]].view;
    }
    for (int j = 0; j < g.m; j++) {
      pars.push_back(GBuf::input(parity0[j]));
      if (v != 1 || j == g.m - 1) out[g.parity[j]] = pars[j].view;
    }
    s.ec->apply_delta(in, out);
    for (auto &[shard, b] : ins) b.verify(c, s.name, shard, false);
    for (int j = 0; j < g.m; j++) {
      const bool passed = v != 1 || j == g.m - 1;
      pars[j].verify(c, s.name, g.parity[j], passed);
      if (passed) {
        results[v]->keys.insert(g.parity[j]);
        results[v]->out[g.parity[j]] = pars[j].bytes();
      }
    }
  }
  return r;
}

// ---- pattern shortlists ---------------------------------------------------

// subsets of {0..n-1} of size 0..max_size, by size then lexicographically,
// at most `cap` of them
std::vector<std::set<int>> subsets_upto(int n, int max_size, size_t cap) {
  std::vector<std::set<int>> all;
  for (int sz = 0; sz <= max_size && sz <= n; sz++) {
    std::vector<int> idx(sz);
    for (int i = 0; i < sz; i++) idx[i] = i;
    for (;;) {
      if (all.size() >= cap) return all;
      all.emplace_back(idx.begin(), idx.end());
      int p = sz - 1;
      while (p >= 0 && idx[p] == n - sz + p) p--;
      if (p < 0) break;
      idx[p]++;
      for (int q = p + 1; q < sz; q++) idx[q] = idx[q - 1] + 1;
    }
  }
  return all;
}

// exactly m erasures: first ceil(m/2) data and last floor(m/2) parity shards
std::set<int> m_pattern(const Geometry &g) {
  std::set<int> e;
  const int nd = std::min((g.m + 1) / 2, g.k), np = g.m - nd;
  for (int i = 0; i < nd; i++) e.insert(g.data[i]);
  for (int j = 0; j < np; j++) e.insert(g.parity[g.m - 1 - j]);
  return e;
}

std::set<int> plus_one(const Geometry &g, std::set<int> e) {
  for (int i = 0; i < g.k; i++)
    if (e.insert(g.data[i]).second) return e;
  for (int j = 0; j < g.m; j++)
    if (e.insert(g.parity[j]).second) return e;
  return e;
}

// ---- the steps ------------------------------------------------------------

std::set<int> all_shards(const Geometry &g) {
  std::set<int> s;
  for (int i = 0; i < g.n; i++) s.insert(i);
  return s;
}

template <typename T>
void cmp_scalar(const std::string &call, T ref, T dut) {
  if (ref != dut) {
    std::ostringstream o;
    o << "ref=" << ref << " dut=" << dut;
    fail(call, o.str());
  }
  g_compared[g_step]++;
}

void step_shape(Side &ref, Side &dut, unsigned W) {
  g_step = "shape";
  cmp_scalar("get_chunk_count", ref.ec->get_chunk_count(),
             dut.ec->get_chunk_count());
  cmp_scalar("get_data_chunk_count", ref.ec->get_data_chunk_count(),
             dut.ec->get_data_chunk_count());
  cmp_scalar("get_sub_chunk_count", ref.ec->get_sub_chunk_count(),
             dut.ec->get_sub_chunk_count());
  const auto &rm = ref.ec->get_chunk_mapping(), &dm = dut.ec->get_chunk_mapping();
  cmp_scalar("get_chunk_mapping size", rm.size(), dm.size());
  for (size_t i = 0; i < rm.size(); i++)
    cmp_scalar("get_chunk_mapping[" + std::to_string(i) + "]", (int)rm[i],
               (int)dm[i]);
  for (unsigned w : {1u, 15u, 17u, 4095u, W, W + 1})
    cmp_scalar("get_chunk_size(" + std::to_string(w) + ")",
               ref.ec->get_chunk_size(w), dut.ec->get_chunk_size(w));
}

Geometry geometry_of(Side &ref, unsigned W) {
  Geometry g;
  g.n = (int)ref.ec->get_chunk_count();
  g.k = (int)ref.ec->get_data_chunk_count();
  g.m = g.n - g.k;
  const auto &cm = ref.ec->get_chunk_mapping();
  for (int raw = 0; raw < g.n; raw++) {
    int shard = cm.size() > (size_t)raw ? (int)cm[raw] : raw;
    (raw < g.k ? g.data : g.parity).push_back(shard);
  }
  g.C = ref.ec->get_chunk_size(W);
  return g;
}

void step_minimum(Side &ref, Side &dut, const Geometry &g) {
  g_step = "minimum";
  auto missing = subsets_upto(g.n, g.m, 64);
  std::set<int> too_many;
  for (int i = 0; i <= g.m; i++) too_many.insert(i);
  missing.push_back(too_many);
  std::vector<std::set<int>> wants;
  for (int i = 0; i < g.n; i++) wants.push_back({i});
  wants.emplace_back(g.data.begin(), g.data.end());
  for (auto &miss : missing) {
    shard_id_set avail;
    for (int i = 0; i < g.n; i++)
      if (!miss.count(i)) avail.insert(i);
    for (auto &want : wants) {
      const std::string call =
          "minimum_to_decode want=" + set_name(want) + " missing=" + set_name(miss);
      shard_id_set rmin, dmin;
      shard_id_map<std::vector<std::pair<int, int>>> rsub(g.n), dsub(g.n);
      int rr = ref.ec->minimum_to_decode(to_shard_set(want), avail, rmin, &rsub);
      int dr = dut.ec->minimum_to_decode(to_shard_set(want), avail, dmin, &dsub);
      if (rr != dr)
        fail(call, "return code ref=" + std::to_string(rr) +
                       " dut=" + std::to_string(dr));
      if (rr == 0) {
        for (int i = 0; i < g.n; i++) {
          if (rmin.contains(i) != dmin.contains(i))
            fail(call, "minimum set differs at shard=" + std::to_string(i));
          if (rsub.contains(i) != dsub.contains(i) ||
              (rsub.contains(i) && rsub.at(i) != dsub.at(i)))
            fail(call, "sub-chunk list differs at shard=" + std::to_string(i));
        }
      }
      g_compared[g_step]++;
    }
  }
}

// full-width encode on both sides; returns REF's chunks by shard id
std::vector<Bytes> encode_both(Side &ref, Side *dut, const Geometry &g,
                               const Bytes &in, const std::string &call) {
  Res r = do_encode(ref, g, all_shards(g), in, call);
  if (dut) compare(call, r, do_encode(*dut, g, all_shards(g), in, call));
  if (r.rc || (int)r.out.size() != g.n)
    fail(call, "ref could not encode: rc=" + std::to_string(r.rc));
  std::vector<Bytes> chunks(g.n);
  for (auto &[shard, b] : r.out) chunks[shard] = b;
  return chunks;
}

void step_encode_want(Side &ref, Side &dut, const Geometry &g, const Bytes &in) {
  g_step = "encode_want";
  const std::set<int> wants[2] = {{g.parity[g.m - 1]},
                                  {g.data[0], g.parity[0]}};
  for (auto &want : wants) {
    const std::string call = "encode want=" + set_name(want);
    compare(call, do_encode(ref, g, want, in, call),
            do_encode(dut, g, want, in, call));
  }
}

void step_encode_chunks(Side &ref, Side &dut, const Geometry &g,
                        const std::vector<Bytes> &data) {
  g_step = "encode_chunks";
  std::vector<int> all_par;
  for (int j = 0; j < g.m; j++) all_par.push_back(j);
  struct Case {
    const char *name;
    std::set<int> absent, via_out;
    std::vector<int> parities;
  } cases[] = {
      {"encode_chunks(a) all data, all parity", {}, {}, all_par},
      {"encode_chunks(b) data 1 absent", {1}, {}, all_par},
      {"encode_chunks(c) data 0 via out, last parity only", {}, {0}, {g.m - 1}},
  };
  for (auto &c : cases)
    compare(c.name,
            do_encode_chunks(ref, g, data, c.absent, c.via_out, c.parities,
                             c.name),
            do_encode_chunks(dut, g, data, c.absent, c.via_out, c.parities,
                             c.name));
}

std::vector<GBuf> hold(const std::vector<Bytes> &chunks) {
  std::vector<GBuf> h;
  for (auto &c : chunks) h.push_back(GBuf::input(c));
  return h;
}

void decode_case(Side &ref, Side &dut, const Geometry &g,
                 const std::vector<Bytes> &enc, const std::vector<GBuf> &rh,
                 const std::vector<GBuf> &dh, const std::set<int> &want,
                 const std::set<int> &erased) {
  const std::string call =
      "decode want=" + set_name(want) + " erased=" + set_name(erased);
  Res r = do_decode(ref, g, rh, want, erased, call);
  compare(call, r, do_decode(dut, g, dh, want, erased, call));
  if (r.rc == 0)
    for (int s : want) cmp_bytes(call, s, enc[s], r.out.at(s), "encoded", "ref");
}

void step_decode(Side &ref, Side &dut, const Geometry &g,
                 const std::vector<Bytes> &enc, bool singles_only) {
  std::vector<GBuf> rh = hold(enc), dh = hold(enc);
  std::vector<std::set<int>> patterns;
  for (int i = 0; i < g.n; i++) patterns.push_back({i});
  if (!singles_only) {
    if (g.m >= 2)
      for (int i = 0; i < g.n; i++)
        for (int j = i + 1; j < g.n; j++) patterns.push_back({i, j});
    if (g.m >= 3) {
      // m-1 erasures: with m = 6 the five outputs split into launches of
      // four and one, the six of the next pattern into four and two
      std::set<int> e = m_pattern(g);
      e.erase(g.parity[g.m - 1]);
      patterns.push_back(e);
    }
    patterns.push_back(m_pattern(g));
    patterns.push_back(plus_one(g, m_pattern(g)));
  }
  for (auto &e : patterns) {
    decode_case(ref, dut, g, enc, rh, dh, e, e);
    if (e.size() < 2) continue;
    decode_case(ref, dut, g, enc, rh, dh, {*e.begin()}, e);
    for (int i = 0; i < g.k; i++)
      if (!e.count(g.data[i])) {
        std::set<int> more = e;
        more.insert(g.data[i]);
        decode_case(ref, dut, g, enc, rh, dh, more, e);
        break;
      }
  }
}

void step_decode_chunks(Side &ref, Side &dut, const Geometry &g,
                        const std::vector<Bytes> &enc) {
  g_step = "decode_chunks";
  std::vector<GBuf> rh = hold(enc), dh = hold(enc);
  const std::set<int> e = m_pattern(g);
  int present = 0;
  while (e.count(present)) present++;
  struct Case {
    const char *name;
    std::set<int> neither, left_out;
  } cases[] = {
      {"decode_chunks(a) every erased shard in out", {}, {}},
      {"decode_chunks(b) last erased shard in neither map", {*e.rbegin()}, {}},
      {"decode_chunks(c) a present shard left out of in", {}, {present}},
  };
  for (auto &c : cases) {
    const std::string call = std::string(c.name) + " erased=" + set_name(e);
    Res r = do_decode_chunks(ref, g, rh, e, c.neither, c.left_out, call);
    compare(call, r, do_decode_chunks(dut, g, dh, e, c.neither, c.left_out, call));
    if (r.rc == 0)
      for (auto &[s, b] : r.out) cmp_bytes(call, s, enc[s], b, "encoded", "ref");
  }
}

bool claims_delta(Side &s) {
  return s.ec->get_supported_optimizations() &
         ErasureCodeInterface::FLAG_EC_PLUGIN_PARITY_DELTA_OPTIMIZATION;
}

void step_delta(Side &ref, Side &dut, const Geometry &g,
                const std::vector<Bytes> &data, Rng &rng, bool dut_alone) {
  g_step = "delta";
  if (!claims_delta(dut) || (!dut_alone && !claims_delta(ref))) {
    g_skipped[g_step] = "plugin does not claim parity delta";
    return;
  }
  // the full re-encode comes from REF, or from DUT itself when it has no twin
  Side &enc = dut_alone ? dut : ref;
  std::vector<int> all_par;
  for (int j = 0; j < g.m; j++) all_par.push_back(j);
  auto parity_of = [&](const std::vector<Bytes> &d, const std::string &call) {
    Res r = do_encode_chunks(enc, g, d, {}, {}, all_par, call);
    if (r.rc) fail(call, "re-encode failed: rc=" + std::to_string(r.rc));
    std::vector<Bytes> p;
    for (int j = 0; j < g.m; j++) p.push_back(r.out.at(g.parity[j]));
    return p;
  };
  const std::vector<Bytes> parity0 = parity_of(data, "delta: old parity");
  std::vector<std::set<int>> sets = {{1}};
  if (g.k > 1) sets.push_back({0, g.k - 1});
  for (auto &set : sets) {
    const std::string call = "overwrite data" + set_name(set);
    std::map<int, Bytes> fresh;
    std::vector<Bytes> updated = data;
    for (int i : set) updated[i] = fresh[i] = rng.bytes(g.C);
    const Bytes junk = rng.bytes(g.C);
    const std::vector<Bytes> want = parity_of(updated, call + " re-encode");
    DeltaRes d = do_delta(dut, g, data, fresh, parity0, junk, call);
    if (!dut_alone) {
      DeltaRes r = do_delta(ref, g, data, fresh, parity0, junk, call);
      compare(call + " encode_delta", r.deltas, d.deltas);
      compare(call + " apply_delta(a)", r.all, d.all);
      compare(call + " apply_delta(b)", r.last_only, d.last_only);
      compare(call + " apply_delta(c)", r.with_parity_entry,
              d.with_parity_entry);
    }
    // delta and re-encode must agree, whatever REF's delta path does
    for (int j = 0; j < g.m; j++) {
      const int shard = g.parity[j];
      cmp_bytes(call + " apply_delta(a) vs re-encode", shard, want[j],
                d.all.out.at(shard), "reencode", "dut");
      cmp_bytes(call + " apply_delta(c) vs re-encode", shard, want[j],
                d.with_parity_entry.out.at(shard), "reencode", "dut");
    }
    cmp_bytes(call + " apply_delta(b) vs re-encode", g.parity[g.m - 1],
              want[g.m - 1], d.last_only.out.at(g.parity[g.m - 1]), "reencode",
              "dut");
    g_compared[g_step]++;
  }
}

void run_width(Side &ref, Side &dut, const Options &o, unsigned W) {
  auto on = [&](const char *step) {
    return o.only.empty() || o.only.count(step);
  };
  g_width = W;
  g_view_off = GUARD;
  step_shape(ref, dut, W);
  const Geometry g = geometry_of(ref, W);
  g_chunk_of[W] = g.C;
  if (on("minimum")) step_minimum(ref, dut, g);

  Rng rng{o.seed ^ ((uint64_t)W << 20)};
  const Bytes in = rng.bytes(W);
  std::vector<Bytes> data;
  for (int i = 0; i < g.k; i++) data.push_back(rng.bytes(g.C));
  const uint64_t delta_seed = rng.next();

  for (size_t off : {GUARD, GUARD + 16}) {
    g_view_off = off;
    g_step = "encode";
    const std::vector<Bytes> enc =
        encode_both(ref, on("encode") ? &dut : nullptr, g, in, "encode all");
    if (on("encode_want")) step_encode_want(ref, dut, g, in);
    if (on("encode_chunks")) step_encode_chunks(ref, dut, g, data);
    if (on("decode")) {
      g_step = "decode";
      step_decode(ref, dut, g, enc, false);
    }
    if (on("decode_chunks")) step_decode_chunks(ref, dut, g, enc);
    if (on("delta")) {
      Rng drng{delta_seed};
      step_delta(ref, dut, g, data, drng, o.delta_vs_reencode);
    }
    if (on("repeat")) {
      // same instances, same shapes: resident params, cached decode plans
      // and captured graphs are reused instead of built
      g_step = "repeat";
      encode_both(ref, &dut, g, in, "encode all, again");
      step_decode(ref, dut, g, enc, true);
      // a zeros chunk changes the launch params the cache held
      Bytes zeroed = in;
      for (size_t i = 2 * (size_t)g.C; i < zeroed.size() && i < 3 * (size_t)g.C; i++)
        zeroed[i] = 0;
      encode_both(ref, &dut, g, zeroed, "encode all, data 2 zeroed");
    }
  }
}

int make_codec(const Options &o, const std::string &plugin,
               const ErasureCodeProfile &profile, ErasureCodeInterfaceRef *ec) {
  ErasureCodeProfile p = profile;  // factory may write defaults
  std::stringstream ss;
  int r = ErasureCodePluginRegistry::instance().factory(plugin, o.dir, p, ec,
                                                        &ss);
  if (r) std::cerr << plugin << ": factory failed (" << r << ") " << ss.str() << "\n";
  return r;
}

}  // namespace

int main(int argc, char **argv) {
  Options o;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--delta-vs-reencode") {
      o.delta_vs_reencode = true;
      continue;
    }
    if (a == "-h" || a == "--help" || i + 1 >= argc) return usage();
    const std::string v = argv[++i];
    if (a == "-d") {
      o.dir = v;
    } else if (a == "--ref") {
      o.ref = v;
    } else if (a == "--dut") {
      o.dut = v;
    } else if (a == "-P" || a == "--ref-P" || a == "--dut-P") {
      auto eq = v.find('=');
      if (eq == std::string::npos) return usage();
      if (a != "--dut-P") o.ref_profile[v.substr(0, eq)] = v.substr(eq + 1);
      if (a != "--ref-P") o.dut_profile[v.substr(0, eq)] = v.substr(eq + 1);
    } else if (a == "-s") {
      o.widths.push_back((unsigned)std::strtoul(v.c_str(), nullptr, 10));
    } else if (a == "--seed") {
      o.seed = std::strtoull(v.c_str(), nullptr, 0);
    } else if (a == "--only") {
      std::stringstream ss(v);
      std::string step;
      while (std::getline(ss, step, ',')) {
        if (std::find_if(std::begin(STEPS), std::end(STEPS), [&](const char *s) {
              return step == s;
            }) == std::end(STEPS)) {
          std::cerr << "unknown step " << step << "\n";
          return usage();
        }
        o.only.insert(step);
      }
    } else {
      std::cerr << "unknown option " << a << "\n";
      return usage();
    }
  }
  if (o.ref.empty() || o.dut.empty() || o.widths.empty()) return usage();
  for (unsigned w : o.widths)
    if (!w) return usage();
  if (o.delta_vs_reencode) o.only = {"delta"};
  o.only.erase("shape");  // always runs
  const bool all_steps = o.only.empty();

  int rc = 0;
  {
    Side ref{"ref", nullptr}, dut{"dut", nullptr};
    if (make_codec(o, o.ref, o.ref_profile, &ref.ec) ||
        make_codec(o, o.dut, o.dut_profile, &dut.ec))
      return 2;
    try {
      for (unsigned W : o.widths) run_width(ref, dut, o, W);
    } catch (const Diff &) {
      rc = 1;
    } catch (const std::exception &e) {
      std::cout << where("exception") << " " << e.what() << std::endl;
      rc = 1;
    }
  }
  if (rc) return rc;
  for (auto &[width, chunk] : g_chunk_of)
    std::cout << "WIDTH " << width << " chunk=" << chunk << "\n";
  for (const char *step : STEPS) {
    if (!all_steps && std::string(step) != "shape" && !o.only.count(step))
      continue;
    if (g_skipped.count(step))
      std::cout << "STEP " << step << " skipped=" << g_skipped[step] << "\n";
    else
      std::cout << "STEP " << step << " compared=" << g_compared[step] << "\n";
  }
  std::cout << "DIFF_OK" << std::endl;
  return 0;
}
