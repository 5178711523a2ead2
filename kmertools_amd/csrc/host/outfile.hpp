// outfile.hpp - one output file of a command.  open() and close() return "" or the text the CLI prints after "Error: ";
// the first failed write sticks (what is written afterwards goes nowhere, close() reports it once), and the destructor
// closes what an early return left open.  An OutFile that was never opened swallows everything and closes clean, so a
// command that leaves a file out under some flag does not open it and need not ask again at every write.
#pragma once
#include <cstdio>
#include <string>
#include <vector>

namespace kthost {

class OutFile {
  public:
    static constexpr size_t FLUSH_AT = 1u << 22;  // text() goes to the file once it holds this much
    OutFile() = default;
    OutFile(const OutFile &) = delete;
    OutFile &operator=(const OutFile &) = delete;
    ~OutFile() { (void)close(); }

    std::string open(const std::string &path) {
        (void)close();
        path_ = path, failed_ = false;
        f_ = fopen(path.c_str(), "wb");
        return f_ ? "" : error();
    }
    bool is_open() const { return f_ != nullptr; }
    bool failed() const { return failed_; }
    // the message of a failure of this file (a site with a text of its own asks failed() and says that instead)
    std::string error() const { return "Unable to write to file: " + path_; }
    // The file's text buffer: ask for it anew for every line or record appended - a buffer that has reached FLUSH_AT is
    // written out first -, and close() writes the rest.
    std::string &text() {
        if (buf_.size() >= FLUSH_AT) flush();
        return buf_;
    }
    // straight to the file, behind whatever text() still holds; false once the file has failed
    bool write(const char *p, size_t n) { return flush(), put(p, n), !failed_; }
    bool write(const std::string &s) { return write(s.data(), s.size()); }
    bool write(const std::vector<std::string> &pieces) {
        flush();
        for (const std::string &p : pieces) put(p.data(), p.size());
        return !failed_;
    }
    // for a writer that calls fwrite itself (AsyncWriter): its failures are its own, close() still reports fclose's
    FILE *stream() { return flush(), f_; }
    // "" or the message, once: a second close(), or one of a file that never opened, has nothing to report
    std::string close() {
        if (!f_) return "";
        flush();
        if (fclose(f_) != 0) failed_ = true;
        f_ = nullptr;
        return failed_ ? error() : "";
    }

  private:
    void flush() { put(buf_.data(), buf_.size()), buf_.clear(); }
    void put(const char *p, size_t n) {
        if (f_ && !failed_ && n && fwrite(p, 1, n, f_) != n) failed_ = true;
    }
    FILE *f_ = nullptr;
    bool failed_ = false;
    std::string path_, buf_;
};

}  // namespace kthost
