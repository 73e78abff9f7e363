// kr_inspect.cpp — `krepp inspect` on the host: the statistics of an index in their canonical form (kr_index_stats_cpu) and the
// report text (kr_format_inspect).  Reference: Index::display_info (src/index.cpp:172-186), FlatHT::display_info
// (src/table.cpp:262-270), CRecord::display_info (src/record.cpp:257-276), Tree::stream_nwk_basic (src/phytree.cpp:66-82).
// Nothing here touches HIP: the device twin is kr_index_stats.hip, which returns the same arrays.
#include "kr_common.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace {

// The library's file suffix as the builders write it (src/krepp.cpp:72-87): -m<M>r<R>-frac / -no_frac
std::string lib_suffix(const kr_index_view* v, uint32_t lib)
{
  const kr_lib_view& lv = v->libs[lib];
  return "-m" + std::to_string(v->m) + "r" + std::to_string(lv.r) + (lv.frac ? "-frac" : "-no_frac");
}

void lib_stats_release(kr_lib_stats* L)
{
  free(L->mer_value), free(L->mer_freq), free(L->deg_value), free(L->deg_freq), free(L->se_count), free(L->se_outdeg);
  L->mer_value = L->mer_freq = L->deg_value = L->deg_freq = L->se_count = L->se_outdeg = nullptr;
  L->n_mer = L->n_deg = 0;
}

// (value, how many of vals[1 .. n) have it), ascending by value: the reference's "histogram of a histogram"
int value_histogram(const std::vector<uint64_t>& vals, kr_lib_stats* L, int which)
{
  std::vector<uint64_t> s(vals.begin() + std::min<size_t>(1, vals.size()), vals.end()), value, freq;
  std::sort(s.begin(), s.end());
  for (size_t i = 0; i < s.size(); ++i) {
    if (i == 0 || s[i] != s[i - 1]) value.push_back(s[i]), freq.push_back(0);
    freq.back()++;
  }
  return kr::lib_stats_set_list(L, which, value.data(), freq.data(), value.size());
}

int keep_array(const std::vector<uint64_t>& v, uint64_t** out)
{
  *out = (uint64_t*)malloc(std::max<size_t>(1, v.size()) * 8);
  if (!*out) return kr::fail(KR_ERR_NOMEM, "kr_index_stats: out of memory");
  if (!v.empty()) memcpy(*out, v.data(), v.size() * 8);
  return KR_OK;
}

// One library; the first colour id >= nsubsets in cmer, then in a child of se_to_pse[1 ..], ends it
int lib_stats_host(const kr_index_view* v, uint32_t lib, uint32_t flags, kr_lib_stats* L)
{
  const kr_lib_view& lv = v->libs[lib];
  const uint32_t ns = lv.nsubsets;
  std::vector<uint64_t> count(ns, 0), outdeg(ns, 0);
  for (uint64_t i = 0; i < lv.nkmers; ++i) {
    const uint32_t se = lv.cmer[2 * i + 1];
    if (se >= ns) return kr::stats_bad_id(v, lib, "cmer", i, se);
    count[se]++;
  }
  for (uint32_t ix = 1; ix < ns; ++ix) {
    const uint32_t a = lv.pse[2 * (uint64_t)ix], b = lv.pse[2 * (uint64_t)ix + 1];
    if (a >= ns || b >= ns) return kr::stats_bad_id(v, lib, "se_to_pse", ix, a >= ns ? a : b);
    outdeg[a]++, outdeg[b]++;
  }
  if (int rc = value_histogram(count, L, 0)) return rc;
  if (int rc = value_histogram(outdeg, L, 1)) return rc;
  if (flags & KR_STATS_KEEP_COUNTS) {
    if (int rc = keep_array(count, &L->se_count)) return rc;
    if (int rc = keep_array(outdeg, &L->se_outdeg)) return rc;
  }
  return KR_OK;
}

// Tree::stream_nwk_basic: children in their order, the raw label, ":<blen>" in the default ostream form unless NaN
void nwk_basic(const kr_host_index* hx, const std::vector<std::vector<uint32_t>>& kids, uint32_t se, bool root, std::string& o)
{
  if (!kids[se].empty()) {
    o += "(";
    for (size_t i = 0; i < kids[se].size(); ++i) {
      nwk_basic(hx, kids, kids[se][i], false, o);
      if (i + 1 < kids[se].size()) o += ",";
    }
    o += ")";
  }
  o += kr_host_index_node_label(hx, se);
  const double blen = kr_host_index_node_blen(hx, se);
  if (!std::isnan(blen)) {
    char buf[64];
    snprintf(buf, sizeof buf, "%g", blen);
    o += ":";
    o += buf;
  }
  if (root) o += ";";
}

} // namespace

int kr::stats_bad_id(const kr_index_view* v, uint32_t lib, const char* array, uint64_t pos, uint32_t value)
{
  return kr::fail(KR_ERR_FORMAT, "library " + lib_suffix(v, lib) + ": " + array + "[" + std::to_string(pos) + "] names colour id " + std::to_string(value) +
                                   ", but the colour record has " + std::to_string(v->libs[lib].nsubsets));
}

int kr::index_stats_alloc(const kr_index_view* v, kr_index_stats* out)
{
  out->nlibs = 0;
  out->libs = (kr_lib_stats*)calloc(std::max<uint32_t>(1, v->nlibs), sizeof(kr_lib_stats));
  if (!out->libs) return kr::fail(KR_ERR_NOMEM, "kr_index_stats: out of memory");
  out->nlibs = v->nlibs;
  for (uint32_t i = 0; i < v->nlibs; ++i) {
    kr_lib_stats& L = out->libs[i];
    L.nkmers = v->libs[i].nkmers, L.nsubsets = v->libs[i].nsubsets, L.r = v->libs[i].r, L.frac = v->libs[i].frac;
  }
  return KR_OK;
}

int kr::lib_stats_set_list(kr_lib_stats* L, int which, const uint64_t* value, const uint64_t* freq, uint64_t n)
{
  uint64_t* a = (uint64_t*)malloc(std::max<uint64_t>(1, n) * 8);
  uint64_t* b = (uint64_t*)malloc(std::max<uint64_t>(1, n) * 8);
  if (!a || !b) {
    free(a), free(b);
    return kr::fail(KR_ERR_NOMEM, "kr_index_stats: out of memory");
  }
  if (n) memcpy(a, value, n * 8), memcpy(b, freq, n * 8);
  if (which == 0) free(L->mer_value), free(L->mer_freq), L->mer_value = a, L->mer_freq = b, L->n_mer = n;
  else free(L->deg_value), free(L->deg_freq), L->deg_value = a, L->deg_freq = b, L->n_deg = n;
  return KR_OK;
}

extern "C" {

int kr_index_stats_cpu(const kr_index_view* v, uint32_t flags, kr_index_stats* out)
{
  kr::clear_error();
  if (!v || !out || (v->nlibs && !v->libs)) return kr::fail(KR_ERR_ARG, "kr_index_stats_cpu: null argument");
  memset(out, 0, sizeof(*out));
  if (flags & KR_VIEW_DEVICE) return kr::fail(KR_ERR_ARG, "kr_index_stats_cpu: the view must be in host memory");
  for (uint32_t i = 0; i < v->nlibs; ++i)
    if ((v->libs[i].nkmers && !v->libs[i].cmer) || (v->libs[i].nsubsets && !v->libs[i].pse))
      return kr::fail(KR_ERR_ARG, "kr_index_stats_cpu: null argument");
  if (int rc = kr::index_stats_alloc(v, out)) return rc;
  for (uint32_t i = 0; i < v->nlibs; ++i)
    if (int rc = lib_stats_host(v, i, flags, &out->libs[i])) {
      kr_index_stats_free(out);
      return rc;
    }
  return KR_OK;
}

void kr_index_stats_free(kr_index_stats* s)
{
  if (!s) return;
  for (uint32_t i = 0; s->libs && i < s->nlibs; ++i) lib_stats_release(&s->libs[i]);
  free(s->libs);
  s->libs = nullptr, s->nlibs = 0;
}

int kr_format_inspect(const kr_host_index* hx, const kr_index_stats* st, char** text, uint64_t* len)
{
  kr::clear_error();
  if (!hx || !st || !text || !len) return kr::fail(KR_ERR_ARG, "kr_format_inspect: null argument");
  *text = nullptr, *len = 0;
  kr_index_view v;
  kr_host_index_view(hx, &v);
  if (st->nlibs != v.nlibs) return kr::fail(KR_ERR_ARG, "kr_format_inspect: the statistics are not this index's");
  std::string o = "Backbone tree: ";
  if (v.wbackbone) {
    std::vector<std::vector<uint32_t>> kids(v.tree_nnodes + 1);
    uint32_t root = 0;
    for (uint32_t se = 1; se <= v.tree_nnodes; ++se) { // post-order numbers: a node's children in ascending order are in file order
      const uint32_t p = kr_host_index_node_parent(hx, se);
      if (p && p <= v.tree_nnodes) kids[p].push_back(se);
      else root = se;
    }
    if (root) nwk_basic(hx, kids, root, true, o);
    o += "\n";
  } else {
    o += "NA\n";
  }
  // a frac library of residue r serves the keys 0 .. r, any other its own r (src/index.cpp:144-157); one block per key
  std::map<uint32_t, uint32_t> by_key;
  for (uint32_t i = 0; i < v.nlibs; ++i) {
    if (v.libs[i].frac)
      for (uint32_t q = 0; q <= v.libs[i].r; ++q) by_key[q] = i;
    else
      by_key[v.libs[i].r] = i;
  }
  for (const auto& kv : by_key) {
    const std::string key = std::to_string(kv.first);
    const kr_lib_stats& L = st->libs[kv.second];
    o += "======= Partial index: " + key + " =======\n";
    o += kr_host_index_lib_info(hx, kv.second);
    o += key + "\tNUM_COLORS\t" + std::to_string(L.nsubsets - 1) + "\n"; // (32-bit, as the reference's nsubsets - 1)
    for (uint64_t q = 0; q < L.n_mer; ++q) o += key + "\tMER_COUNT\t" + std::to_string(L.mer_value[q]) + "\t" + std::to_string(L.mer_freq[q]) + "\n";
    for (uint64_t q = 0; q < L.n_deg; ++q) o += key + "\tOUTDEGREE_COUNT\t" + std::to_string(L.deg_value[q]) + "\t" + std::to_string(L.deg_freq[q]) + "\n";
  }
  char* p = (char*)malloc(o.size() + 1);
  if (!p) return kr::fail(KR_ERR_NOMEM, "kr_format_inspect: out of memory");
  memcpy(p, o.c_str(), o.size() + 1);
  *text = p, *len = o.size();
  return KR_OK;
}

} // extern "C"
