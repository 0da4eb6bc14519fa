// Stand-alone program over the host mirror's readers alone (no engine, no device): the two facts a CsrBlock
// keeps about itself -- every value's bits are 1.0f; every row is one entry per field in field order -- as
// CsrBlock::push, the token path of CsrStream, load_csr, CsrData::slice / gather and a split block compute
// them (ftrl-ffm_amd/host/types.h).  Built by tests/test_implicit_ones_host.py with g++, plain and with
// -fsanitize=address,undefined.
//   usage: implicit_ones <scratch directory>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../ftrl-ffm_amd/host/csr_reader.h"
#include "../ftrl-ffm_amd/host/csr_stream.h"
#include "../ftrl-ffm_amd/host/types.h"

static int n_ok = 0, n_failed = 0;
static void expect(bool cond, const std::string &what) {
  std::printf("%s %s\n", cond ? "ok  " : "FAIL", what.c_str());
  (cond ? n_ok : n_failed)++;
}
static void write(const std::string &path, const std::string &text) {
  std::ofstream f(path, std::ios::binary);
  f << text;
}

constexpr int F = 3;  // fields of the hand-written blocks

// what a block claims: (values all ones, one entry per field for F fields)
struct Facts { bool ones, regular; };
static bool is(const CsrBlock &b, Facts want) { return b.all_ones == want.ones && b.one_entry_per_field(F) == want.regular; }
// ... and what its arrays say (the second pass the readers must not need)
static Facts recount(const CsrBlock &b) {
  Facts f{true, true};
  for (float v : b.val) f.ones = f.ones && is_one_bits(v);
  for (int r = 0; r < b.n_rows(); r++) {
    f.regular = f.regular && b.row_ptr[r + 1] - b.row_ptr[r] == F;
    for (int p = b.row_ptr[r]; p < b.row_ptr[r + 1]; p++) f.regular = f.regular && b.field[p] == p - b.row_ptr[r];
  }
  return f;
}

struct Case { const char *name, *text; Facts want; };

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const std::string dir = argv[1], path = dir + "/d.ffm";
  const float ulp_up = std::nextafterf(1.0f, 2.0f);
  char ulp_text[64];
  std::snprintf(ulp_text, sizeof ulp_text, "%.9g", ulp_up);  // parses back to 1.0f + ulp exactly

  const std::string one_ulp = std::string("1 0:1:1 1:2:") + ulp_text + " 2:3:1\n0 0:4:1 1:5:1 2:6:1\n";
  const Case cases[] = {
      {"all ones", "1 0:1:1 1:2:1 2:3:1\n0 0:4:1.0 1:5:1.000 2:6:+1\n", {true, true}},
      {"one -1.0f", "1 0:1:1 1:2:1 2:3:1\n0 0:4:1 1:5:-1 2:6:1\n", {false, true}},
      {"one 1.0f + ulp", one_ulp.c_str(), {false, true}},
      {"rows out of field order", "1 0:1:1 1:2:1 2:3:1\n0 0:4:1 2:6:1 1:5:1\n", {true, false}},
      {"a row with a missing field", "1 0:1:1 1:2:1 2:3:1\n0 0:4:1 2:6:1\n", {true, false}},
      {"a multi-valued field", "1 0:1:1 1:2:1 2:3:1\n0 0:4:1 1:5:1 1:7:1 2:6:1\n", {true, false}},
      {"a value of zero is dropped: the row lacks its field", "1 0:1:1 1:2:0 2:3:1\n", {true, false}},
      {"an empty row among regular ones", "1 0:1:1 1:2:1 2:3:1\n0\n", {true, false}},
      {"scientific notation of one", "1 0:1:1e0 1:2:10e-1 2:3:0.1e1\n", {true, true}},
  };

  // ---- CsrBlock::push
  {
    CsrBlock b;
    expect(!b.all_ones && !b.all_ordered, "push: a block nobody cleared claims nothing");
    b.clear();
    expect(is(b, {true, true}) && b.n_rows() == 0, "push: an empty block is all ones and regular");
    b.push(Sample{{{0, 1, 1.0f}, {1, 2, 1.0f}, {2, 3, 1.0f}}, 1});
    expect(is(b, {true, true}), "push: all ones");
    CsrBlock c = b;
    c.push(Sample{{{0, 4, 1.0f}, {1, 5, -1.0f}, {2, 6, 1.0f}}, 0});
    expect(is(c, {false, true}), "push: one -1.0f");
    c = b;
    c.push(Sample{{{0, 4, 1.0f}, {1, 5, ulp_up}, {2, 6, 1.0f}}, 0});
    expect(is(c, {false, true}), "push: one 1.0f + ulp");
    c = b;
    c.push(Sample{{{0, 4, 1.0f}, {2, 6, 1.0f}, {1, 5, 1.0f}}, 0});
    expect(is(c, {true, false}), "push: rows out of field order");
    c = b;
    c.push(Sample{{{0, 4, 1.0f}, {2, 6, 1.0f}}, 0});
    expect(is(c, {true, false}), "push: a row with a missing field");
    c = b;
    c.push(Sample{{{0, 4, 1.0f}, {1, 5, 1.0f}, {1, 7, 1.0f}, {2, 6, 1.0f}}, 0});
    expect(is(c, {true, false}), "push: a multi-valued field");
    c = b;
    c.push(Sample{{}, 0});
    expect(is(c, {true, false}), "push: an empty row among regular ones");
    c.clear();
    expect(is(c, {true, true}), "push: clear() starts over");
    c.push(Sample{{{0, 4, 2.0f}}, 0});
    c.forget_facts();
    expect(!c.all_ones && !c.one_entry_per_field(1), "forget_facts: claims nothing");
  }

  // ---- the token path: CsrStream::next, load_csr + slice / gather
  for (const Case &k : cases) {
    write(path, k.text);
    ftrl::CsrStream st(path, "libffm", 2);
    CsrBlock b;
    const size_t got = st.next(100, b);
    const Facts seen = recount(b);
    expect(got > 0 && is(b, k.want) && seen.ones == k.want.ones && seen.regular == k.want.regular, std::string("stream: ") + k.name);
    const ftrl::CsrData d = ftrl::load_csr(path, "libffm", 2);
    CsrBlock s;
    d.slice(0, d.n_rows(), s);
    expect(d.flags.size() == d.n_rows() && is(s, k.want), std::string("load_csr + slice: ") + k.name);
    std::vector<int> idx(d.n_rows());
    for (size_t i = 0; i < idx.size(); i++) idx[i] = static_cast<int>(idx.size() - 1 - i);
    CsrBlock g;
    d.gather(idx.data(), idx.size(), g, 1);
    expect(is(g, k.want), std::string("load_csr + gather: ") + k.name);
  }

  // ---- an empty block: no rows at all
  {
    write(path, "\n\n");
    ftrl::CsrStream st(path, "libffm", 1);
    CsrBlock b;
    expect(st.next(10, b) == 0 && is(b, {true, true}), "stream: an empty block");
    const ftrl::CsrData d = ftrl::load_csr(path, "libffm", 1);
    CsrBlock g;
    d.gather(nullptr, 0, g, 1);
    expect(d.n_rows() == 0 && is(g, {true, true}), "gather: an empty block");
  }

  // ---- blocks cut out of one file: the facts are the block's rows', not the file's
  {
    // rows 0-3 regular ones, row 4 carries 0.5, row 5 lacks a field, rows 6-7 regular ones
    write(path,
          "1 0:1:1 1:2:1 2:3:1\n0 0:4:1 1:5:1 2:6:1\n1 0:1:1 1:2:1 2:3:1\n0 0:4:1 1:5:1 2:6:1\n"
          "1 0:1:1 1:2:0.5 2:3:1\n0 0:4:1 2:6:1\n1 0:1:1 1:2:1 2:3:1\n0 0:4:1 1:5:1 2:6:1\n");
    ftrl::CsrStream st(path, "libffm", 2);
    CsrBlock b;
    expect(st.next(4, b) == 4 && is(b, {true, true}), "stream blocks: rows 0-3");
    expect(st.next(1, b) == 1 && is(b, {false, true}), "stream blocks: row 4 (a value of 0.5)");
    expect(st.next(1, b) == 1 && is(b, {true, false}), "stream blocks: row 5 (a missing field)");
    expect(st.next(4, b) == 2 && is(b, {true, true}), "stream blocks: rows 6-7 after the others");
    st.rewind();
    expect(st.next(100, b, /*max_nnz=*/7) == 2 && is(b, {true, true}) && b.val.size() == 6, "stream blocks: cut by the entry budget");
    expect(st.next(100, b) == 6 && is(b, {false, false}), "stream blocks: the rest");
    const ftrl::CsrData d = ftrl::load_csr(path, "libffm", 3);
    CsrBlock s;
    d.slice(0, 4, s);
    expect(is(s, {true, true}), "slice: rows 0-3");
    d.slice(3, 5, s);
    expect(is(s, {false, true}), "slice: rows 3-4");
    d.slice(5, 8, s);
    expect(is(s, {true, false}), "slice: rows 5-7");
    const int pick[4] = {7, 0, 6, 2}, with4[2] = {1, 4}, with5[3] = {5, 3, 0};
    CsrBlock g;
    d.gather(pick, 4, g, 1);
    expect(is(g, {true, true}) && recount(g).ones && recount(g).regular, "gather: regular rows of ones, shuffled");
    d.gather(with4, 2, g, 1);
    expect(is(g, {false, true}), "gather: with row 4");
    d.gather(with5, 3, g, 1);
    expect(is(g, {true, false}), "gather: with row 5");
    d.gather(pick, 4, g, 1);
    expect(is(g, {true, true}), "gather: a reused block starts over");
    // a split block: every run of its rows inherits its facts
    CsrBlock whole, part;
    d.slice(0, 4, whole);
    part.inherit_facts(whole);
    expect(is(part, {true, true}), "split: a part of a regular block of ones");
    d.slice(0, 8, whole);
    part.inherit_facts(whole);
    expect(is(part, {false, false}), "split: a part of a mixed block claims nothing more than the whole");
  }

  // ---- libsvm rows have no fields: never "one entry per field", values still noted
  {
    write(path, "1 3:1 9:1\n0 4:1\n");
    ftrl::CsrStream st(path, "libsvm", 1);
    CsrBlock b;
    expect(st.next(10, b) == 2 && b.all_ones && !b.one_entry_per_field(2), "libsvm: all ones, no field order");
  }

  std::printf("%d ok, %d failed\n", n_ok, n_failed);
  return n_failed ? 1 : 0;
}
