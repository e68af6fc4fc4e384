// cli/text_io.hpp -- the text writers of the drop-in tools: writeData(file, data, delim[, precision]) of
// util/text_io.hxx:103-133 as hmt/main_merge_order_pb.cxx:37-38 and hmt/main_merge_order_bc.cxx:148-157 call it.  Every element is
// followed by the delimiter; a precision <= 0 keeps the stream's default (6 significant digits).  No HIP dependency: the
// CPU suite builds cli/text_io_check from this header and compares its bytes with the reference's own writers
// (oracle/_ref/ref_misc, tests/test_oracle_vs_ref.py).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

namespace cli {

[[noreturn]] inline void perr(const std::string& msg) {   // glia_base.hxx:66-69
  std::cerr << msg << std::endl;
  exit(EXIT_FAILURE);
}

inline void writeOrder(const std::string& file, const std::vector<uint32_t>& o, int64_t n) {
  std::ofstream os(file);
  if (!os) perr("Error: cannot create file " + file);
  for (int64_t i = 0; i < n; ++i) os << o[3 * i] << " " << o[3 * i + 1] << " " << o[3 * i + 2] << "\n";
}
inline void writeDoubles(const std::string& file, const double* d, int64_t n, int precision = -1) {
  std::ofstream os(file);
  if (!os) perr("Error: cannot create file " + file);
  if (precision > 0) os.precision(precision);
  for (int64_t i = 0; i < n; ++i) os << d[i] << "\n";
}
inline void writeRows(const std::string& file, const double* d, int64_t rows, int cols, int precision) {
  std::ofstream os(file);
  if (!os) perr("Error: cannot create file " + file);
  if (precision > 0) os.precision(precision);
  for (int64_t i = 0; i < rows; ++i) { for (int k = 0; k < cols; ++k) os << d[i * cols + k] << " "; os << "\n"; }
}

// readData of a matrix (util/text_io.hxx; pred_rf's and train_rf's feature and label files): one row per line, values separated by blanks
// rows of a feature file; *dim = their common length (0 for an empty file)
inline std::vector<double> readRows(const std::string& file, int64_t* rows, int* dim) {
  std::ifstream is(file);
  if (!is) perr("Error: cannot open file " + file);
  std::vector<double> v;
  std::string line;
  *rows = 0; *dim = 0;
  while (std::getline(is, line)) {
    const char* p = line.c_str();
    int n = 0;
    for (;;) {
      char* end = nullptr;
      const double x = strtod(p, &end);       // also reads "nan" / "inf", which operator>> refuses
      if (end == p) break;
      v.push_back(x); ++n; p = end;
    }
    while (*p == ' ' || *p == '\t' || *p == '\r') ++p;
    if (*p) perr("Error: invalid value in data file " + file);
    if (n == 0) continue;                     // blank line
    if (*rows > 0 && n != *dim) perr("Error: invalid data file dimension in " + file);
    *dim = n; ++*rows;
  }
  return v;
}

}  // namespace cli
