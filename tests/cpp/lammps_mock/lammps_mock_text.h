// MOCK of text_file_reader.h, tokenizer.h and the file helpers of utils.h, written from the public LAMMPS developer
// documentation (see lammps_mock.h).  Included by lammps_mock.h under LAMMPS_MOCK_FMT only: the recipe that compiles
// the reference's CPU sources needs it, the plugin adapter does not.
#pragma once

#include <algorithm>
#include <cctype>
#include <cstring>
#include <exception>

#define TOKENIZER_DEFAULT_SEPARATORS " \t\r\n\f"

namespace LAMMPS_NS {

class TokenizerException : public std::exception {
  std::string message;

 public:
  TokenizerException(const std::string &msg, const std::string &token)
      : message(token.empty() ? msg : msg + ": '" + token + "'")
  {
  }
  const char *what() const noexcept override { return message.c_str(); }
};
class InvalidIntegerException : public TokenizerException {
 public:
  explicit InvalidIntegerException(const std::string &token) : TokenizerException("Not a valid integer number", token) {}
};
class InvalidFloatException : public TokenizerException {
 public:
  explicit InvalidFloatException(const std::string &token)
      : TokenizerException("Not a valid floating-point number", token)
  {
  }
};

// Words of a string between any of the separator characters; next_*() throws TokenizerException when none is left,
// next_int() / next_double() when the word is not wholly a number.
class ValueTokenizer {
  std::string text, separators;
  size_t start = 0;

 public:
  ValueTokenizer(const std::string &str, const std::string &seps = TOKENIZER_DEFAULT_SEPARATORS)
      : text(str), separators(seps)
  {
  }
  bool has_next() const { return text.find_first_not_of(separators, start) != std::string::npos; }
  std::string next_string()
  {
    const size_t b = text.find_first_not_of(separators, start);
    if (b == std::string::npos) throw TokenizerException("No more tokens", "");
    size_t e = text.find_first_of(separators, b);
    if (e == std::string::npos) e = text.size();
    start = e;
    return text.substr(b, e - b);
  }
  int next_int()
  {
    const std::string w = next_string();
    char *end = nullptr;
    const long v = std::strtol(w.c_str(), &end, 10);
    if (end == w.c_str() || *end) throw InvalidIntegerException(w);
    return (int) v;
  }
  double next_double()
  {
    const std::string w = next_string();
    char *end = nullptr;
    const double v = std::strtod(w.c_str(), &end);
    if (end == w.c_str() || *end) throw InvalidFloatException(w);
    return v;
  }
  size_t count() const
  {
    size_t n = 0, p = 0;
    while ((p = text.find_first_not_of(separators, p)) != std::string::npos) {
      n++;
      p = text.find_first_of(separators, p);
      if (p == std::string::npos) break;
    }
    return n;
  }
  void skip(int n = 1)
  {
    while (n-- > 0) next_string();
  }
};

class FileReaderException : public std::exception {
  std::string message;

 public:
  explicit FileReaderException(const std::string &msg) : message(msg) {}
  const char *what() const noexcept override { return message.c_str(); }
};

// Lines of an already open file, one fgets() each into a buffer of `bufsize` characters and nothing read ahead (the
// caller may go on reading the FILE itself); with ignore_comments everything from '#' on is cut, the newline with it;
// lines without a word are skipped; nullptr at the end of the file.  The file is not closed.  set_bufsize() takes any
// size, as documented ("adjust line buffer size"): a line longer than the buffer comes back in pieces.
class TextFileReader {
  FILE *fp;
  std::string filetype;
  int bufsize = 1024;
  char *line;

 public:
  bool ignore_comments = true;
  TextFileReader(FILE *file, std::string type) : fp(file), filetype(std::move(type)), line(new char[1024]) {}
  TextFileReader(const TextFileReader &) = delete;
  TextFileReader &operator=(const TextFileReader &) = delete;
  virtual ~TextFileReader() { delete[] line; }
  void set_bufsize(int newsize)
  {
    if (newsize < 2) newsize = 2;
    delete[] line;
    line = new char[newsize];
    bufsize = newsize;
  }
  char *next_line(int nparams = 0)
  {
    size_t n = 0;
    int words = 0;
    line[0] = '\0';
    while (words == 0 || words < nparams) {
      if ((int) n + 1 >= bufsize) break;
      char *p = std::fgets(line + n, bufsize - (int) n, fp);
      if (!p) return words > 0 ? line : nullptr;
      if (ignore_comments && (p = std::strchr(line + n, '#'))) *p = '\0';
      words = (int) ValueTokenizer(line).count();
      if (words > 0) n = std::strlen(line);   // (a wordless line is overwritten by the next one)
    }
    return line;
  }
};
class PotentialFileReader;   // potential_file_reader.h: only its name is needed

namespace utils {
inline std::string lowercase(const std::string &s)
{
  std::string r(s);
  std::transform(r.begin(), r.end(), r.begin(), [](unsigned char c) { return (char) std::tolower(c); });
  return r;
}
// the file as named, else under $LAMMPS_POTENTIALS; nullptr when there is none
inline FILE *open_potential(const std::string &name, LAMMPS *, int *)
{
  const std::string path = get_potential_file_path(name);
  return path.empty() ? nullptr : std::fopen(path.c_str(), "r");
}
inline double numeric(const char *, int, const std::string &str, bool, LAMMPS *lmp)
{
  char *end = nullptr;
  const double v = std::strtod(str.c_str(), &end);
  if (str.empty() || end == str.c_str() || *end)
    lmp->error->all("", 0, "Expected floating point parameter instead of '{}' in input script or data file", str);
  return v;
}
inline void sfread(const char *, int, void *s, size_t size, size_t num, FILE *fp, const char *filename, Error *error)
{
  if (num == 0) return;
  if (std::fread(s, size, num, fp) != num)
    error->one("", 0, "Unexpected {} while reading file {}", std::feof(fp) ? "end of file" : "error",
               filename ? filename : "(unknown)");
}
}   // namespace utils

}   // namespace LAMMPS_NS
