// dx_model_dump.cpp -- prints what dx_model_load derives from model blobs, on the host:
//
//   dx_model_dump BLOB...
//
// For each blob file a "# <file name>" line, then one line per table, sorted by name: name,
// dtype, element count and the 64-bit FNV-1a hash of the bytes -- every entry of
// dx_model::hf and ::hi, body_chain, the scalars of DevModel ("dm": everything before the
// first pointer, then nbitem, nbplane, ldl_nslot, ldl_sync), the three LDS layouts and the
// two capacities.  A blob that does not load prints "error: <dx_last_error>" instead.
//
// Stand-alone it links dexterity_amd/csrc/dx_model.hip alone: no HIP library, no GPU
// (tests/test_model_tables_host.py).  With DX_DUMP_HOOK defined it is a hook: included at
// the end of a translation unit that already defines dx_model, as
// tools/record_model_tables_golden.py does to record the golden from an older revision.
#ifndef DX_DUMP_HOOK
#include "../../dexterity_amd/csrc/dx_host.h"
#endif

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

static uint64_t dump_fnv1a(const void* p, size_t n) {
  uint64_t h = 14695981039346656037ull;
  for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
  return h;
}

static void dump_model(const dx_model* m) {
  std::map<std::string, std::string> lines;
  auto item = [&](const std::string& name, const char* dtype, size_t count, const void* p, size_t bytes) {
    char buf[96];
    snprintf(buf, sizeof(buf), " %s %zu %016llx", dtype, count, (unsigned long long)dump_fnv1a(p, bytes));
    lines[name] = name + buf;
  };
  for (const auto& kv : m->hf) item(kv.first, "f32", kv.second.size(), kv.second.data(), kv.second.size() * 4);
  for (const auto& kv : m->hi) item(kv.first, "i32", kv.second.size(), kv.second.data(), kv.second.size() * 4);
  item("body_chain", "u64", m->body_chain.size(), m->body_chain.data(), m->body_chain.size() * 8);
  std::vector<unsigned char> dm((const unsigned char*)&m->dm, (const unsigned char*)&m->dm + offsetof(DevModel, body_parent));
  const int tail[4] = {m->dm.nbitem, m->dm.nbplane, m->dm.ldl_nslot, (int)m->dm.ldl_sync};
  dm.insert(dm.end(), (const unsigned char*)tail, (const unsigned char*)tail + sizeof(tail));
  item("dm", "u8", dm.size(), dm.data(), dm.size());
  item("lds", "i32", sizeof(Lds) / 4, &m->lds, sizeof(Lds));
  item("lds_mid", "i32", sizeof(Lds) / 4, &m->lds_mid, sizeof(Lds));
  item("lds_hi", "i32", sizeof(Lds) / 4, &m->lds_hi, sizeof(Lds));
  item("ncon_max", "i32", 1, &m->ncon_max, 4);
  item("nefc_max", "i32", 1, &m->nefc_max, 4);
  for (const auto& kv : lines) printf("%s\n", kv.second.c_str());
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; a++) {
    const char* base = argv[a];
    for (const char* c = argv[a]; *c; c++)
      if (*c == '/') base = c + 1;
    printf("# %s\n", base);
    FILE* f = fopen(argv[a], "rb");
    if (!f) {
      fprintf(stderr, "dx_model_dump: cannot open %s\n", argv[a]);
      return 2;
    }
    std::vector<unsigned char> blob;
    unsigned char buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) blob.insert(blob.end(), buf, buf + n);
    fclose(f);
    dx_model* m = dx_model_load(blob.data(), blob.size());
    if (!m) {
      printf("error: %s\n", dx_last_error());
      continue;
    }
    dump_model(m);
    delete m;  // (never uploaded: nothing of dx_model_free's to release)
  }
  return 0;
}
