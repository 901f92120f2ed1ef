// Host check of csrc/csv_parse.h (tests/test_csv_parse_host.py builds and runs it):
//   g++ -O2 -ffp-contract=off -std=c++17 tools/csv_parse_check.cpp -o csv_parse_check
//   csv_parse_check < one cell per line > "kind bits" per line
// kind is csvp_cell's (0 INT, 1 FLOAT, 2 EMPTY, 3 DEFER), bits the result's 16
// hex digits (0 for a deferred cell).  A line's '\n' is not part of the cell;
// every other byte is, a '\r' included.
#include "../clustering-driven-replication-strategy_amd/csrc/csv_parse.h"

#include <cstdio>
#include <string>
#include <vector>

int main() {
  std::vector<char> in;
  char buf[1 << 16];
  size_t got;
  while ((got = std::fread(buf, 1, sizeof buf, stdin)) > 0) in.insert(in.end(), buf, buf + got);
  std::string out;
  size_t s = 0;
  for (size_t i = 0; i < in.size(); ++i) {
    if (in[i] != '\n') continue;
    double v = 0.0;
    const int kind = csvp_cell(reinterpret_cast<const uint8_t*>(in.data()) + s, (int)(i - s), &v);
    uint64_t bits = 0;
    if (kind != CSVP_DEFER) memcpy(&bits, &v, 8);
    char line[40];
    std::snprintf(line, sizeof line, "%d %016llx\n", kind, (unsigned long long)bits);
    out += line;
    s = i + 1;
  }
  std::fwrite(out.data(), 1, out.size(), stdout);
  return 0;
}
