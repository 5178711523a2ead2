// kmertools (GPU drop-in) - command line with the reference's `comp oligo`, `comp cgr -k` and
// `ctr` flags (kmertools/src/args.rs:70-130, 208-236; dispatcher :239-368) and `cov`
// (args.rs:132-172, :299-325).  clap conventions are kept: kebab-case long flags, the
// auto-derived short flags, `--flag=value`, `-k4`.  `min`: args.rs:172-205, :326-352.  `filter` (a k-mer read
// filter, not in the reference) follows the same conventions, and so do `compare` (two inputs' k-mer tables side by side)
// and `profile` (per-position k-mer counts and per-sequence medians) and `setop` (intersect / subtract / union / xor of two
// inputs' k-mer tables) and `sketch` (MinHash sketches and Mash distances) and `graph` (de Bruijn adjacency of the counted
// k-mers) and `unitigs` (that graph's maximal unitigs) and `hetmers` (the heterozygous k-mer pairs) and `thread` (reads mapped onto those unitigs) and `card` (a HyperLogLog estimate of the distinct k-mers, which
// also sizes the tables of the others: --estimate-size).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <map>
#include <string>
#include <vector>

#include "computers.hpp"
#include "outfile.hpp"
#include "seqio.hpp"

using namespace kthost;

namespace {

struct Spec {
    char shortf;
    const char *longf;
    bool takes_value;
};

[[noreturn]] void usage_error(const std::string &msg) {
    fprintf(stderr, "error: %s\n\nFor more information, try '--help'.\n", msg.c_str());
    exit(2);
}

// parses argv[from..] against `specs`; returns long-name -> value ("true" for switches)
std::map<std::string, std::string> parse_flags(int argc, char **argv, int from, const std::vector<Spec> &specs,
                                               const char *help) {
    std::map<std::string, std::string> out;
    auto find_long = [&](const std::string &n) -> const Spec * {
        for (const auto &s : specs)
            if (n == s.longf) return &s;
        return nullptr;
    };
    auto find_short = [&](char c) -> const Spec * {
        for (const auto &s : specs)
            if (c == s.shortf) return &s;
        return nullptr;
    };
    for (int i = from; i < argc; i++) {
        std::string a = argv[i];
        if (a == "-h" || a == "--help") {
            fputs(help, stdout);
            exit(0);
        }
        if (a.rfind("--", 0) == 0) {
            std::string name = a.substr(2), val;
            bool has_val = false;
            const size_t eq = name.find('=');
            if (eq != std::string::npos) {
                val = name.substr(eq + 1);
                name = name.substr(0, eq);
                has_val = true;
            }
            const Spec *s = find_long(name);
            if (!s) usage_error("unexpected argument '--" + name + "' found");
            if (s->takes_value) {
                if (!has_val) {
                    if (i + 1 >= argc) usage_error("a value is required for '--" + name + "' but none was supplied");
                    val = argv[++i];
                }
                out[s->longf] = val;
            } else {
                out[s->longf] = "true";
            }
        } else if (a.size() >= 2 && a[0] == '-' && a != "-") {
            for (size_t j = 1; j < a.size(); j++) {
                const Spec *s = find_short(a[j]);
                if (!s) usage_error(std::string("unexpected argument '-") + a[j] + "' found");
                if (s->takes_value) {
                    std::string val = a.substr(j + 1);
                    if (!val.empty() && val[0] == '=') val = val.substr(1);
                    if (val.empty()) {
                        if (i + 1 >= argc)
                            usage_error(std::string("a value is required for '-") + a[j] + "' but none was supplied");
                        val = argv[++i];
                    }
                    out[s->longf] = val;
                    break;
                }
                out[s->longf] = "true";
            }
        } else {
            usage_error("unexpected argument '" + a + "' found");
        }
    }
    return out;
}

uint64_t ranged(const std::map<std::string, std::string> &f, const char *name, uint64_t lo, uint64_t hi, bool required,
                uint64_t dflt, bool *present = nullptr) {
    auto it = f.find(name);
    if (present) *present = it != f.end();
    if (it == f.end()) {
        if (required) usage_error(std::string("the following required arguments were not provided:\n  --") + name);
        return dflt;
    }
    char *end = nullptr;
    const unsigned long long v = strtoull(it->second.c_str(), &end, 10);
    if (it->second.empty() || *end) usage_error("invalid value '" + it->second + "' for '--" + name + "': invalid digit found in string");
    if (v < lo || v > hi)
        usage_error("invalid value '" + it->second + "' for '--" + name + "': " + it->second + " is not in " +
                    std::to_string(lo) + "..=" + std::to_string(hi));
    return v;
}

std::string required_str(const std::map<std::string, std::string> &f, const char *name) {
    auto it = f.find(name);
    if (it == f.end()) usage_error(std::string("the following required arguments were not provided:\n  --") + name);
    return it->second;
}

// ---- --estimate-size [--estimate-precision P] of the commands that make a k-mer table ---------------------------------
#define SPEC_ESTIMATE_SIZE {0, "estimate-size", false}
#define SPEC_ESTIMATE_P {0, "estimate-precision", true}
#define HELP_ESTIMATE_(sharded)                                                                                              \
    "      --estimate-size          Size the table from an estimate of the distinct k-mers of the input it is counted\n"    \
    "                               from (one extra walk over that input: HyperLogLog registers on the GPU) instead of\n"   \
    "                               from the input's size alone.  An estimate that proves too small costs one more run\n"   \
    "                               with the input's bound.\n" sharded                                                       \
    "      --estimate-precision <P> The estimate's 2^P registers, 4..16 [default: 14] (needs --estimate-size)\n"
#define HELP_ESTIMATE HELP_ESTIMATE_("")
// (the commands that have --devices)
#define HELP_ESTIMATE_SHARDED \
    HELP_ESTIMATE_("                               Not with --devices above 1: the sharded table keeps its bound.\n")

// ---- --table FILE / --alt-table FILE: a table file (ctr --save-table) in place of counting an input ---------------------------
#define SPEC_TABLE {0, "table", true}
#define SPEC_ALT_TABLE {0, "alt-table", true}
// (`counted`: the flag of the input the table would otherwise be counted from)
#define HELP_TABLE_(flag, counted, sharded)                                                                                  \
    "      " flag " <FILE>           Load the table from this table file (ctr --save-table) instead of counting\n"            \
    "                               " counted ", which is then not given; --k-size must be the file's k.\n"                 \
    "                               Not with --estimate-size" sharded ".\n"
#define HELP_TABLE HELP_TABLE_("--table", "--input", "")
#define HELP_TABLE_CTR HELP_TABLE_("--table", "--input", " or --devices above 1")
#define HELP_TABLE_ALT_INPUT HELP_TABLE_("--table", "--alt-input (default: the input)", "")
#define HELP_TABLE_COV HELP_TABLE_("--table", "--alt-input (default: the input)", " or --devices above 1")
#define HELP_TABLES HELP_TABLE_("--table", "--input (A)", "") \
    "      --alt-table <FILE>       The same for --alt-input (B); either one or both may be table files.\n"

// The flag's checks, before any device work and before the output directory is made: the file is read on the host only
// (kt_table_file_info).  `flag`: "table" or "alt-table"; `counted` / `counted_text`: the flag it stands in for.  Returns the
// file's path, "" without the flag.
std::string table_flag(const std::map<std::string, std::string> &f, int k, const char *flag = "table", const char *counted = "input",
                       const char *counted_text = "--input <INPUT>") {
    const auto it = f.find(flag);
    if (it == f.end()) return "";
    const std::string name = std::string("'--") + flag + " <FILE>'";
    if (f.count(counted)) usage_error("the argument " + name + " cannot be used with '" + counted_text + "'");
    if (f.count("estimate-size")) usage_error("the argument " + name + " cannot be used with '--estimate-size'");
    if (f.count("devices") && ranged(f, "devices", 1, 64, false, 1) > 1)
        usage_error("the argument " + name + " cannot be used with '--devices <N>' above 1");
    int fk = 0;
    if (kt_table_file_info(it->second.c_str(), &fk, nullptr, nullptr, nullptr) != KT_OK)
        usage_error("invalid value '" + it->second + "' for " + name + ": " + kt_last_error());
    if (fk != k)
        usage_error("invalid value '" + std::to_string(k) + "' for '--k-size <K_SIZE>': the table file " + it->second + " holds k = " +
                    std::to_string(fk));
    return it->second;
}

// ---- --prefilter [--prefilter-bits N] of ctr, graph, unitigs and hetmers ---------------------------------------------------------
#define SPEC_PREFILTER {0, "prefilter", false}
#define SPEC_PREFILTER_BITS {0, "prefilter-bits", true}
#define HELP_PREFILTER_(sharded)                                                                                             \
    "      --prefilter              Count in two passes: the first marks the k-mers seen twice in a bit filter on the GPU,\n"  \
    "                               the second counts only those, so that the k-mers seen once (in reads: mostly errors)\n"   \
    "                               take no slot of the table - all but a few false positives, which have count 1.  Every\n"  \
    "                               k-mer seen twice or more has its exact count: with --min-count 2 or above, which the\n"   \
    "                               flag requires, the output is that of a run without it.  Writes {output}/prefilter.stats.\n" \
    "                               Not with --table" sharded ".  KT_PREFILTER_SCALE=<float> scales the table's size.\n"       \
    "      --prefilter-bits <N>     Bits of the filter per k-mer expected in the input [default: 16] (needs --prefilter)\n"
#define HELP_PREFILTER HELP_PREFILTER_("")
#define HELP_PREFILTER_SHARDED HELP_PREFILTER_(" or --devices above 1")

struct PrefilterFlags {
    bool on = false;
    uint64_t bits = 16;
};

// checked with the command's other flags, before any device work and before the output directory is made
PrefilterFlags prefilter_flags(const std::map<std::string, std::string> &f, uint64_t min_count) {
    PrefilterFlags pf;
    pf.on = f.count("prefilter") != 0;
    bool has_bits = false;
    pf.bits = ranged(f, "prefilter-bits", 1, 1ull << 40, false, 16, &has_bits);
    if (has_bits && !pf.on) usage_error("the argument '--prefilter-bits <N>' requires '--prefilter'");
    if (!pf.on) return pf;
    if (min_count < 2)
        usage_error("the argument '--prefilter' requires '--min-count <N>' of 2 or above: the k-mers seen once are what it leaves out");
    if (f.count("table")) usage_error("the argument '--prefilter' cannot be used with '--table <FILE>': nothing is counted");
    if (f.count("devices") && ranged(f, "devices", 1, 64, false, 1) > 1)
        usage_error("the argument '--prefilter' cannot be used with '--devices <N>' above 1");
    return pf;
}

struct EstimateFlags {
    bool on = false;
    int p = 14;
};

// checked with the command's other flags, before any device work
EstimateFlags estimate_flags(const std::map<std::string, std::string> &f) {
    EstimateFlags est;
    est.on = f.count("estimate-size") != 0;
    bool has_p = false;
    est.p = (int)ranged(f, "estimate-precision", KT_CARD_MIN_P, KT_CARD_MAX_P, false, 14, &has_p);
    if (has_p && !est.on) usage_error("the argument '--estimate-precision <P>' requires '--estimate-size'");
    if (est.on && ranged(f, "devices", 1, 64, false, 1) > 1)
        usage_error("the argument '--estimate-size' cannot be used with '--devices <N>' above 1");
    return est;
}

// Runs a table command (run() makes the command's computer and returns its error, "" for none) under the estimate flags.
// An estimate that was too small shows as a full table somewhere in the command: the command then runs once more, from
// the start and in this process, with the plan of a run without the flag - its files are written anew.
template <class Run>
int run_table_command(const EstimateFlags &est, Run run) {
    set_estimate_size(est.on, est.p);
    std::string e = run();
    if (est.on && table_overflowed(e)) {
        fprintf(stderr, "[card] estimate %llu was too small for this input: counting again with the input's bound\n",
                (unsigned long long)estimate_size_taken());
        set_estimate_size(false, est.p);
        e = run();
    }
    if (!e.empty()) {
        fprintf(stderr, "Error: %s\n", e.c_str());
        return 101;
    }
    return 0;
}

const char *HELP_MAIN =
    "kmertools: DNA vectorisation\n\n"
    "k-mer based vectorisation for DNA sequences for\nmetagenomics and AI/ML applications\n"
    "(MI355X build: every subcommand's per-base work runs on the GPU)\n\n"
    "Usage: kmertools <COMMAND>\n\n"
    "Commands:\n"
    "  comp    Generate sequence composition based features\n"
    "  cov     Generates coverage histogram based on the reads\n"
    "  min     Bin reads using minimisers\n"
    "  ctr     Count k-mers\n"
    "  filter  Drop or trim reads by the abundance of their k-mers\n"
    "  correct Repair read errors from the solid k-mers of the table\n"
    "  compare Compare the k-mer counts of two inputs (matrix and set similarity)\n"
    "  profile Per-position k-mer counts and per-sequence min / median / mean / max\n"
    "  setop   Intersect, subtract, union or xor the k-mer sets of two inputs\n"
    "  graph   De Bruijn adjacency, unitig ends and node census of the counted k-mers\n"
    "  unitigs Maximal unitigs of the de Bruijn graph of the counted k-mers\n"
    "  hetmers Heterozygous k-mer pairs of the counted k-mers and their coverage matrix\n"
    "  thread  Map reads onto the unitigs of the counted k-mers (exact k-mer threading), GAF output\n"
    "  sketch  MinHash sketches of sequences and their Mash distances; scaled sketches, containment and ANI\n"
    "  card    Estimate the number of distinct k-mers (HyperLogLog), sizes tables\n"
    "  help    Print this message or the help of the given subcommand(s)\n\n"
    "Options:\n  -h, --help     Print help\n  -V, --version  Print version\n";

const char *HELP_OLIGO =
    "Generate oligonucleotide frequency vectors\n\n"
    "Usage: kmertools comp oligo [OPTIONS] --input <INPUT> --output <OUTPUT>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>      Input file path\n"
    "  -o, --output <OUTPUT>    Output vectors path\n"
    "  -c, --counts             Disable normalisation and output raw counts\n"
    "  -k, --k-size <K_SIZE>    Set k-mer size [default: 3]\n"
    "  -r, --raw-count          Raw counts\n"
    "  -p, --preset <PRESET>    Output type to write [default: spc] [possible values: csv, tsv, spc]\n"
    "  -H, --header             Include header (with k-mer in ACGT format)\n"
    "  -t, --threads <THREADS>  Thread count for computations 0=auto [default: 0]\n"
    "      --device <DEVICE>    GPU index [default: 0]\n"
    "  -h, --help               Print help\n";

const char *HELP_CGR =
    "Generates Chaos Game Representations\n\n"
    "Usage: kmertools comp cgr [OPTIONS] --input <INPUT> --output <OUTPUT>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>        Input file path\n"
    "  -o, --output <OUTPUT>      Output vectors path\n"
    "  -c, --counts               Disable normalisation and output raw counts (only with k-mer mode)\n"
    "  -k, --k-size <K_SIZE>      Set k-mer size or default to full sequence CGR\n"
    "  -v, --vec-size <VEC_SIZE>  Set vector size (output will be a square matrix with N=vecsize)\n"
    "  -t, --threads <THREADS>    Thread count for computations 0=auto [default: 0]\n"
    "      --device <DEVICE>      GPU index [default: 0]\n"
    "  -h, --help                 Print help\n";

const char *HELP_CTR =
    "Count k-mers\n\n"
    "Usage: kmertools ctr [OPTIONS] --input <INPUT> --output <OUTPUT> --k-size <K_SIZE>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>      Input file path\n"
    "  -o, --output <OUTPUT>    Output directory path\n"
    "  -k, --k-size <K_SIZE>    k size for counting\n"
    "  -m, --memory <MEMORY>    Max memory in GB [default: 6] (accepted; the bound is the GPU's free HBM: a table\n"
    "                           that cannot hold every distinct k-mer is filled in several passes over the input)\n"
    "  -a, --acgt               Output ACGT instead of numeric values\n"
    "  -t, --threads <THREADS>  Thread count for computations 0=auto [default: 0]\n"
    "      --device <DEVICE>    GPU index [default: 0]\n"
    "      --devices <N>        Shard the table over N GPUs, --device .. --device + N - 1 [default: 1]\n"
    "      --min-count <N>      Write only k-mers that occur at least N times [default: 1]\n"
    "      --max-count <N>      Write only k-mers that occur at most N times [default: 4294967295]\n"
    "      --histo              Also write the abundance spectrum of the whole table to {output}/kmers.histo\n"
    "                           (lines \"count<TAB>k-mers\", count = 1..H; the last line counts H or more)\n"
    "      --histo-max <H>      Highest count of kmers.histo [default: 10000]\n"
    "      --histo-only         Write kmers.histo and no kmers.counts (implies --histo)\n"
    "      --save-table <FILE>  Also write the k-mers in the count range to this table file (binary, sorted, 6 bytes\n"
    "                           a k-mer at k = 31; one section per pass), which graph, unitigs and hetmers load\n"
    "                           with --table instead of counting again.  Works with --histo-only.  Not with --devices\n"
    "                           above 1.\n"
    HELP_TABLE_CTR
    HELP_ESTIMATE_SHARDED
    HELP_PREFILTER_SHARDED
    "                               With --histo the line of count 1 reads \"1<TAB>0\": a filtered table does not know\n"
    "                               how many k-mers were seen once.\n"
    "  -h, --help               Print help\n";

const char *HELP_COV =
    "Generates coverage histogram based on the reads\n\n"
    "Usage: kmertools cov [OPTIONS] --input <INPUT> --output <OUTPUT>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>          Input file path\n"
    "  -a, --alt-input <ALT_INPUT>  Input file path, for k-mer counting\n"
    "  -o, --output <OUTPUT>        Output directory path\n"
    "  -k, --k-size <K_SIZE>        K size for the coverage histogram [default: 15]\n"
    "  -p, --preset <PRESET>        Output type to write [default: spc] [possible values: csv, tsv, spc]\n"
    "  -s, --bin-size <BIN_SIZE>    Bin size for the coverage histogram [default: 16]\n"
    "  -c, --bin-count <BIN_COUNT>  Number of bins for the coverage histogram [default: 16]\n"
    "  -m, --memory <MEMORY>        Max memory in GB [default: 6] (accepted; the table lives in HBM)\n"
    "      --counts                 Disable normalisation and output raw counts\n"
    "  -t, --threads <THREADS>      Thread count for computations 0=auto [default: 0]\n"
    "      --device <DEVICE>        GPU index [default: 0]\n"
    "      --devices <N>            Shard the table over N GPUs, --device .. --device + N - 1 [default: 1]\n"
    HELP_TABLE_COV
    HELP_ESTIMATE_SHARDED
    "  -h, --help                   Print help\n";

int make_out_dir(const std::string &out) {
    // create_directory(&command.output).unwrap()  (args.rs:300, :354)
    if (mkdir(out.c_str(), 0777) != 0) {
        struct stat st;
        if (stat(out.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) {
            fprintf(stderr, "Error: unable to create directory: %s\n", out.c_str());
            return 101;  // the reference panics here
        }
    }
    return 0;
}

int cmd_cov(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true},    {'a', "alt-input", true}, {'o', "output", true},
                                     {'k', "k-size", true},   {'p', "preset", true},    {'s', "bin-size", true},
                                     {'c', "bin-count", true}, {'m', "memory", true},   {0, "counts", false},
                                     {'t', "threads", true},  {0, "device", true},      {0, "devices", true}, 
                                     SPEC_TABLE, SPEC_ESTIMATE_SIZE, SPEC_ESTIMATE_P};
    const auto f = parse_flags(argc, argv, from, specs, HELP_COV);
    const std::string in = required_str(f, "input"), out = required_str(f, "output");
    const int k = (int)ranged(f, "k-size", 7, 31, false, 15);
    const uint64_t bin_size = ranged(f, "bin-size", 5, ~0ull, false, 16);
    const uint64_t bin_count = ranged(f, "bin-count", 5, ~0ull, false, 16);
    const uint64_t mem = ranged(f, "memory", 6, 128, false, 6);
    const int threads = (int)ranged(f, "threads", 0, 1 << 20, false, 0);
    std::string preset = f.count("preset") ? f.at("preset") : "spc";
    if (preset != "csv" && preset != "tsv" && preset != "spc")
        usage_error("invalid value '" + preset + "' for '--preset <PRESET>'\n  [possible values: csv, tsv, spc]");
    const EstimateFlags est = estimate_flags(f);
    const std::string table = table_flag(f, k, "table", "alt-input", "--alt-input <ALT_INPUT>");
    if (int rc = make_out_dir(out)) return rc;
    const std::string kin = !table.empty() ? table : f.count("alt-input") ? f.at("alt-input") : in;
    for (const std::string &p : table.empty() ? std::vector<std::string>{in, kin} : std::vector<std::string>{in}) {
        if (format_from_path(p) == SeqFormat::Unknown) {  // "-" included: both inputs are read more than once
            fprintf(stderr, "Error: unsupported input extension (expected .fa/.fasta/.fna/.fq/.fastq[.gz]): %s\n", p.c_str());
            return 101;  // SeqFormat::get(...).unwrap()
        }
    }
    const int device = (int)ranged(f, "device", 0, 63, false, 0), devices = (int)ranged(f, "devices", 1, 64, false, 1);
    return run_table_command(est, [&]() -> std::string {  // (101: build_table().unwrap() / unwraps inside compute_coverages)
        CovComputer cov(in, out, k, bin_size, bin_count);
        if (threads > 0) cov.set_threads(threads);
        if (!table.empty()) cov.set_kmer_table(table);
        else if (f.count("alt-input")) cov.set_kmer_path(kin);
        if (f.count("counts")) cov.set_norm(false);
        cov.set_max_memory((double)mem);
        cov.set_delim(preset == "csv" ? "," : preset == "tsv" ? "\t" : " ");
        cov.set_device(device);
        cov.set_devices(devices);
        std::string e = cov.build_table();
        if (e.empty()) e = cov.compute_coverages();
        return e;
    });
}

const char *HELP_MIN =
    "Bin reads using minimisers\n\n"
    "Usage: kmertools min [OPTIONS] --input <INPUT> --output <OUTPUT>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>      Input file path\n"
    "  -o, --output <OUTPUT>    Output vectors path\n"
    "  -m, --m-size <M_SIZE>    Minimiser size [default: 10]\n"
    "  -w, --w-size <W_SIZE>    Window size\n"
    "                           \n"
    "                           0 - emits one minimiser per sequence (useful for sequencing reads)\n"
    "                           w_size must be longer than m_size [default: 0]\n"
    "  -p, --preset <PRESET>    Output type to write [default: s2m] [possible values: s2m, m2s]\n"
    "  -t, --threads <THREADS>  Thread count for computations 0=auto [default: 0]\n"
    "      --device <DEVICE>    GPU index [default: 0]\n"
    "  -h, --help               Print help\n";

int cmd_min(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true},  {'o', "output", true},  {'m', "m-size", true}, {'w', "w-size", true},
                                     {'p', "preset", true}, {'t', "threads", true}, {0, "device", true}};
    const auto f = parse_flags(argc, argv, from, specs, HELP_MIN);
    const std::string in = required_str(f, "input"), out = required_str(f, "output");
    const int m = (int)ranged(f, "m-size", 7, 28, false, 10);
    const uint64_t w = ranged(f, "w-size", 0, ~0ull, false, 0);
    const int threads = (int)ranged(f, "threads", 0, 1 << 20, false, 0);
    const int device = (int)ranged(f, "device", 0, 63, false, 0);
    std::string preset = f.count("preset") ? f.at("preset") : "s2m";
    if (preset != "s2m" && preset != "m2s")
        usage_error("invalid value '" + preset + "' for '--preset <PRESET>'\n  [possible values: s2m, m2s]");
    if (w <= (uint64_t)m && w > 0) {  // args.rs:327-330 (returns normally)
        fprintf(stderr, "Window size must be longer than minimiser size!\n");
        return 0;
    }
    const std::string e = preset == "m2s" ? bin_sequences(w, m, in, out, threads, device)
                                          : seq_to_min(w, m, in, out, threads, device);
    if (!e.empty()) {
        fprintf(stderr, "Error: %s\n", e.c_str());
        return 101;  // the reference unwraps every failure in these two functions
    }
    return 0;
}

int cmd_oligo(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true},    {'o', "output", true},  {'c', "counts", false},
                                     {'k', "k-size", true},   {'r', "raw-count", false}, {'p', "preset", true},
                                     {'H', "header", false},  {'t', "threads", true}, {0, "device", true}};
    const auto f = parse_flags(argc, argv, from, specs, HELP_OLIGO);
    const std::string in = required_str(f, "input"), out = required_str(f, "output");
    const int k = (int)ranged(f, "k-size", 3, 7, false, 3);
    const int threads = (int)ranged(f, "threads", 0, 1 << 20, false, 0);
    std::string preset = f.count("preset") ? f.at("preset") : "spc";
    if (preset != "csv" && preset != "tsv" && preset != "spc")
        usage_error("invalid value '" + preset + "' for '--preset <PRESET>'\n  [possible values: csv, tsv, spc]");
    OligoComputer com(in, out, k, !f.count("raw-count"));  // args.rs:243-248
    if (threads > 0) com.set_threads(threads);
    com.set_norm(!f.count("counts"));
    com.set_header(f.count("header") != 0);
    com.set_delim(preset == "csv" ? "," : preset == "tsv" ? "\t" : " ");
    com.set_device((int)ranged(f, "device", 0, 63, false, 0));
    const std::string e = com.vectorise();
    if (!e.empty()) fprintf(stderr, "Error: %s\n", e.c_str());  // args.rs:260-262 (returns normally)
    return 0;
}

int cmd_cgr(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true},  {'o', "output", true},   {'c', "counts", false},
                                     {'k', "k-size", true}, {'v', "vec-size", true}, {'t', "threads", true},
                                     {0, "device", true}};
    const auto f = parse_flags(argc, argv, from, specs, HELP_CGR);
    const std::string in = required_str(f, "input"), out = required_str(f, "output");
    bool has_k = false, has_v = false;
    const int k = (int)ranged(f, "k-size", 3, 7, false, 0, &has_k);
    const uint64_t v = ranged(f, "vec-size", 0, ~0ull, false, 0, &has_v);
    const int threads = (int)ranged(f, "threads", 0, 1 << 20, false, 0);
    if (!has_k) {
        if (f.count("counts")) {  // args.rs:284-287
            fprintf(stderr, "Error: cannot use counts in whole sequence CGR!\n");
            return 0;
        }
        // args.rs:288-296: vecsize defaults to 1
        CgrComputer cgr(in, out, has_v ? v : 1);
        if (threads > 0) cgr.set_threads(threads);
        cgr.set_device((int)ranged(f, "device", 0, 63, false, 0));
        const std::string e = cgr.vectorise();
        if (e == "Bad nucleotide, unable to proceed") {
            // the reference unwraps this Err inside its worker (cgr.rs:95) and the process panics
            fprintf(stderr, "Error: %s\n", e.c_str());
            return 101;
        }
        if (!e.empty()) fprintf(stderr, "Error: %s\n", e.c_str());
        return 0;
    }
    // default vecsize = (k as f64).powf(4.0).powf(0.5) as u64 = k^2   (args.rs:266-269)
    const uint64_t vecsize = has_v ? v : (uint64_t)k * (uint64_t)k;
    OligoCgrComputer cgr(in, out, k, vecsize);
    if (threads > 0) cgr.set_threads(threads);
    cgr.set_norm(!f.count("counts"));
    cgr.set_device((int)ranged(f, "device", 0, 63, false, 0));
    const std::string e = cgr.vectorise();
    if (!e.empty()) fprintf(stderr, "Error: %s\n", e.c_str());
    return 0;
}

int cmd_ctr(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true},  {'o', "output", true}, {'k', "k-size", true},
                                     {'m', "memory", true}, {'a', "acgt", false},  {'t', "threads", true},
                                     {0, "device", true},   {0, "devices", true},
                                     {0, "min-count", true}, {0, "max-count", true}, {0, "histo", false},
                                     {0, "histo-max", true}, {0, "histo-only", false}, {0, "save-table", true},
                                     SPEC_TABLE, SPEC_ESTIMATE_SIZE, SPEC_ESTIMATE_P, SPEC_PREFILTER, SPEC_PREFILTER_BITS};
    const auto f = parse_flags(argc, argv, from, specs, HELP_CTR);
    // (--table FILE stands in for --input: the table file is dumped, filtered, re-saved)
    const std::string in = f.count("table") && !f.count("input") ? f.at("table") : required_str(f, "input"), out = required_str(f, "output");
    const int k = (int)ranged(f, "k-size", 10, 31, true, 0);
    const uint64_t mem = ranged(f, "memory", 6, 128, false, 6);
    const int threads = (int)ranged(f, "threads", 0, 1 << 20, false, 0);
    // the output filters and the spectrum (jellyfish dump -L/-U and histo --high, kmc -ci/-cx): checked before any device work
    const uint64_t min_count = ranged(f, "min-count", 1, 0xFFFFFFFFull, false, 1);
    const uint64_t max_count = ranged(f, "max-count", 1, 0xFFFFFFFFull, false, 0xFFFFFFFFull);
    if (min_count > max_count)
        usage_error("invalid values for '--min-count' and '--max-count': " + std::to_string(min_count) + " is greater than " +
                    std::to_string(max_count));
    const uint64_t histo_max = ranged(f, "histo-max", 1, (1u << 24) - 1, false, 10000);
    const bool histo_only = f.count("histo-only") != 0, histo = histo_only || f.count("histo") != 0;
    const EstimateFlags est = estimate_flags(f);
    const PrefilterFlags pre = prefilter_flags(f, min_count);
    const std::string table = table_flag(f, k);
    const std::string save_table = f.count("save-table") ? f.at("save-table") : "";
    if (!save_table.empty() && ranged(f, "devices", 1, 64, false, 1) > 1)
        usage_error("the argument '--save-table <FILE>' cannot be used with '--devices <N>' above 1");
    if (int rc = make_out_dir(out)) return rc;
    if (table.empty() && format_from_path(in) == SeqFormat::Unknown) {
        // CountComputer::new unwraps SeqFormat::get (counter/src/lib.rs:38): unknown extension - "-" included - panics
        fprintf(stderr, "Error: unsupported input extension (expected .fa/.fasta/.fna/.fq/.fastq[.gz]): %s\n", in.c_str());
        return 101;
    }
    const int devices = (int)ranged(f, "devices", 1, 64, false, 1), device = (int)ranged(f, "device", 0, 63, false, 0);
    set_prefilter(pre.on, pre.bits, out);
    return run_table_command(est, [&]() -> std::string {  // (101: count()/merge() unwrap in the reference)
        CountComputer ctr(in, out, k);
        ctr.set_devices(devices);
        if (threads > 0) ctr.set_threads(threads);
        if (f.count("acgt")) ctr.set_acgt_output(true);
        ctr.set_max_memory((double)mem);
        ctr.set_device(device);
        ctr.set_count_range((uint32_t)min_count, (uint32_t)max_count);
        if (histo) ctr.set_histo((uint32_t)histo_max, histo_only);
        ctr.set_save_table(save_table);
        ctr.set_input_is_table(!table.empty());
        std::string e = ctr.count();
        if (e.empty()) e = ctr.merge(true);
        return e;
    });
}

const char *HELP_FILTER =
    "Drop or trim reads by the abundance of their k-mers\n\n"
    "A k-mer is solid when min-count <= its count <= max-count in the table counted from --alt-input (default: the\n"
    "input), weak otherwise (an absent k-mer is weak).  Reads without a k-mer are dropped.  Kept records are written in\n"
    "the input's format and order, uncompressed, bytes unchanged (FASTA: the sequence on one line).\n\n"
    "Usage: kmertools filter [OPTIONS] --input <INPUT> --output <OUTPUT> --k-size <K_SIZE>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>          Input file path (reads to filter)\n"
    "  -o, --output <OUTPUT>        Output file path (kept reads)\n"
    "  -k, --k-size <K_SIZE>        k size for counting\n"
    "  -a, --alt-input <ALT_INPUT>  Input file path, for k-mer counting [default: the input]\n"
    "      --min-count <N>          Lowest count of a solid k-mer [default: 2]\n"
    "      --max-count <N>          Highest count of a solid k-mer [default: 4294967295]\n"
    "      --min-solid <F>          Keep a read when at least this fraction of its k-mers is solid [default: 1.0]\n"
    "      --trim                   Instead: cut every read before the last base of its first weak k-mer, drop it\n"
    "                               when less than k bases are left\n"
    "  -m, --memory <MEMORY>        Max memory in GB [default: 6] (accepted; the table lives in HBM)\n"
    "  -t, --threads <THREADS>      Thread count for computations 0=auto [default: 0]\n"
    "      --device <DEVICE>        GPU index [default: 0]\n"
    HELP_TABLE_ALT_INPUT
    HELP_ESTIMATE
    "  -h, --help                   Print help\n";

int cmd_filter(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true},      {'o', "output", true},     {'k', "k-size", true},
                                     {'a', "alt-input", true},  {0, "min-count", true},    {0, "max-count", true},
                                     {0, "min-solid", true},    {0, "trim", false},        {'m', "memory", true},
                                     {'t', "threads", true},    {0, "device", true}, SPEC_TABLE, SPEC_ESTIMATE_SIZE, SPEC_ESTIMATE_P};
    const auto f = parse_flags(argc, argv, from, specs, HELP_FILTER);
    const std::string in = required_str(f, "input"), out = required_str(f, "output");
    const int k = (int)ranged(f, "k-size", 10, 31, true, 0);
    // everything is checked before any device work
    const uint64_t min_count = ranged(f, "min-count", 1, 0xFFFFFFFFull, false, 2);
    const uint64_t max_count = ranged(f, "max-count", 1, 0xFFFFFFFFull, false, 0xFFFFFFFFull);
    if (min_count > max_count)
        usage_error("invalid values for '--min-count' and '--max-count': " + std::to_string(min_count) + " is greater than " +
                    std::to_string(max_count));
    const bool trim = f.count("trim") != 0;
    double min_solid = 1.0;
    if (auto it = f.find("min-solid"); it != f.end()) {
        if (trim) usage_error("the argument '--trim' cannot be used with '--min-solid <F>'");
        char *end = nullptr;
        min_solid = strtod(it->second.c_str(), &end);
        if (it->second.empty() || *end || !(min_solid >= 0.0 && min_solid <= 1.0))
            usage_error("invalid value '" + it->second + "' for '--min-solid': not a number in 0..=1");
    }
    const uint64_t mem = ranged(f, "memory", 6, 128, false, 6);
    const int threads = (int)ranged(f, "threads", 0, 1 << 20, false, 0);
    const int device = (int)ranged(f, "device", 0, 63, false, 0);
    const EstimateFlags est = estimate_flags(f);
    const std::string table = table_flag(f, k, "table", "alt-input", "--alt-input <ALT_INPUT>");
    const std::string kin = !table.empty() ? table : f.count("alt-input") ? f.at("alt-input") : in;
    for (const std::string &p : table.empty() ? std::vector<std::string>{in, kin} : std::vector<std::string>{in}) {
        if (format_from_path(p) == SeqFormat::Unknown) {  // "-" included: both inputs are read more than once
            fprintf(stderr, "Error: unsupported input extension (expected .fa/.fasta/.fna/.fq/.fastq[.gz]): %s\n", p.c_str());
            return 101;
        }
    }
    return run_table_command(est, [&]() -> std::string {
        FilterComputer flt(in, out, k);
        if (threads > 0) flt.set_threads(threads);
        if (!table.empty()) flt.set_kmer_table(table);
        else flt.set_kmer_path(kin);
        flt.set_count_range((uint32_t)min_count, (uint32_t)max_count);
        flt.set_min_solid(min_solid);
        flt.set_trim(trim);
        flt.set_max_memory((double)mem);
        flt.set_device(device);
        return flt.filter();
    });
}

const char *HELP_CORRECT =
    "Repair read errors from the solid k-mers of the table\n\n"
    "A k-mer is solid when min-count <= its count <= max-count in the table counted from --alt-input (default: the\n"
    "input).  A base that lies in a solid k-mer of its read is trusted.  Any other base is rewritten when exactly one\n"
    "other nucleotide there makes at least min-support of the k-mers over it solid; a base with several such nucleotides\n"
    "is left alone, and so is a read that would need more than max-corrections repairs.  Substitutions only, decided\n"
    "from the uncorrected read; two errors closer than k with no solid k-mer between them stay.  Every record is\n"
    "written, in the input's format and order, uncompressed (FASTA: the sequence on one line; FASTQ: qualities unchanged).\n"
    "When the table does not fit the device memory it is counted in several passes, twice over; per-base counts and\n"
    "supports of the whole input (8 bytes per base) are then kept in host memory - refused when larger than --memory.\n\n"
    "Usage: kmertools correct [OPTIONS] --input <INPUT> --output <OUTPUT> --k-size <K_SIZE>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>          Input file path (reads to correct)\n"
    "  -o, --output <OUTPUT>        Output file path (every read, repaired where possible)\n"
    "  -k, --k-size <K_SIZE>        k size for counting\n"
    "  -a, --alt-input <ALT_INPUT>  Input file path, for k-mer counting [default: the input]\n"
    "      --min-count <N>          Lowest count of a solid k-mer [default: 2]\n"
    "      --max-count <N>          Highest count of a solid k-mer [default: 4294967295]\n"
    "      --min-support <N>        Solid k-mers a replacement must make, 1..255 [default: 1]\n"
    "      --max-corrections <N>    Leave a read with more repairable bases than this as it is, 0 = no limit [default: 0]\n"
    "      --stats <FILE>           Write reads, bases, reads_corrected, bases_corrected, positions_ambiguous and\n"
    "                               reads_over_limit as name<TAB>value lines\n"
    "  -m, --memory <MEMORY>        Max memory in GB [default: 6] (the table lives in HBM; bounds the per-base arrays\n"
    "                               kept across the passes of an out-of-core count)\n"
    "  -t, --threads <THREADS>      Thread count for computations 0=auto [default: 0]\n"
    "      --device <DEVICE>        GPU index [default: 0]\n"
    HELP_TABLE_ALT_INPUT
    HELP_ESTIMATE
    "  -h, --help                   Print help\n";

int cmd_correct(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true},       {'o', "output", true},          {'k', "k-size", true},
                                     {'a', "alt-input", true},   {0, "min-count", true},         {0, "max-count", true},
                                     {0, "min-support", true},   {0, "max-corrections", true},   {0, "stats", true},
                                     {'m', "memory", true},      {'t', "threads", true},         {0, "device", true}, 
                                     SPEC_TABLE, SPEC_ESTIMATE_SIZE, SPEC_ESTIMATE_P};
    const auto f = parse_flags(argc, argv, from, specs, HELP_CORRECT);
    const std::string in = required_str(f, "input"), out = required_str(f, "output");
    const int k = (int)ranged(f, "k-size", 10, 31, true, 0);
    // everything is checked before any device work
    const uint64_t min_count = ranged(f, "min-count", 1, 0xFFFFFFFFull, false, 2);
    const uint64_t max_count = ranged(f, "max-count", 1, 0xFFFFFFFFull, false, 0xFFFFFFFFull);
    if (min_count > max_count)
        usage_error("invalid values for '--min-count' and '--max-count': " + std::to_string(min_count) + " is greater than " +
                    std::to_string(max_count));
    const uint64_t min_support = ranged(f, "min-support", 1, 255, false, 1);
    const uint64_t max_corrections = ranged(f, "max-corrections", 0, 0xFFFFFFFFull, false, 0);
    const uint64_t mem = ranged(f, "memory", 6, 128, false, 6);
    const int threads = (int)ranged(f, "threads", 0, 1 << 20, false, 0);
    const int device = (int)ranged(f, "device", 0, 63, false, 0);
    const EstimateFlags est = estimate_flags(f);
    const std::string table = table_flag(f, k, "table", "alt-input", "--alt-input <ALT_INPUT>");
    const std::string kin = !table.empty() ? table : f.count("alt-input") ? f.at("alt-input") : in;
    for (const std::string &p : table.empty() ? std::vector<std::string>{in, kin} : std::vector<std::string>{in}) {
        if (format_from_path(p) == SeqFormat::Unknown) {  // "-" included: both inputs are read more than once
            fprintf(stderr, "Error: unsupported input extension (expected .fa/.fasta/.fna/.fq/.fastq[.gz]): %s\n", p.c_str());
            return 101;
        }
    }
    return run_table_command(est, [&]() -> std::string {
        CorrectComputer cor(in, out, k);
        if (threads > 0) cor.set_threads(threads);
        if (!table.empty()) cor.set_kmer_table(table);
        else cor.set_kmer_path(kin);
        cor.set_count_range((uint32_t)min_count, (uint32_t)max_count);
        cor.set_min_support((uint32_t)min_support);
        cor.set_max_corrections((uint32_t)max_corrections);
        if (f.count("stats")) cor.set_stats_path(f.at("stats"));
        cor.set_max_memory((double)mem);
        cor.set_device(device);
        return cor.correct();
    });
}

const char *HELP_COMPARE =
    "Compare the k-mer counts of two inputs (matrix and set similarity)\n\n"
    "Counts the canonical k-mers of both inputs and writes {output}/compare.matrix: line r (r = 0..max-a) holds max-b + 1\n"
    "tab-separated numbers, the number of k-mers that occur r times in the input and c times in the alt input (0: absent;\n"
    "the last line and the last column: that count or more; the first number of the first line is 0), and\n"
    "{output}/compare.stats: distinct_a, distinct_b, shared, occurrences_a, occurrences_b, shared_min, jaccard,\n"
    "containment_a, containment_b and weighted_jaccard, one \"name<TAB>value\" line each.\n\n"
    "Usage: kmertools compare [OPTIONS] --input <INPUT> --alt-input <ALT_INPUT> --output <OUTPUT> --k-size <K_SIZE>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>          Input file path (the rows)\n"
    "  -a, --alt-input <ALT_INPUT>  Input file path to compare with (the columns)\n"
    "  -o, --output <OUTPUT>        Output directory path\n"
    "  -k, --k-size <K_SIZE>        k size for counting\n"
    "      --max-a <N>              Highest count of the rows; the last row counts N or more [default: 1000]\n"
    "      --max-b <N>              Highest count of the columns; the last column counts N or more [default: 100]\n"
    "  -m, --memory <MEMORY>        Max memory in GB [default: 6] (accepted; the tables live in HBM: when both cannot\n"
    "                               hold every distinct k-mer, the inputs are counted in several passes)\n"
    "  -t, --threads <THREADS>      Thread count for computations 0=auto [default: 0]\n"
    "      --device <DEVICE>        GPU index [default: 0]\n"
    HELP_TABLES
    HELP_ESTIMATE
    "  -h, --help                   Print help\n";

int cmd_compare(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true},  {'a', "alt-input", true}, {'o', "output", true},
                                     {'k', "k-size", true}, {0, "max-a", true},       {0, "max-b", true},
                                     {'m', "memory", true}, {'t', "threads", true},   {0, "device", true}, 
                                     SPEC_TABLE, SPEC_ALT_TABLE, SPEC_ESTIMATE_SIZE, SPEC_ESTIMATE_P};
    const auto f = parse_flags(argc, argv, from, specs, HELP_COMPARE);
    // (--table FILE stands in for --input, --alt-table FILE for --alt-input)
    const std::string in = f.count("table") ? f.at("table") : required_str(f, "input");
    const std::string alt = f.count("alt-table") ? f.at("alt-table") : required_str(f, "alt-input"), out = required_str(f, "output");
    const int k = (int)ranged(f, "k-size", 10, 31, true, 0);
    // everything is checked before any device work
    const uint64_t max_a = ranged(f, "max-a", 1, (1u << 24) - 1, false, 1000);
    const uint64_t max_b = ranged(f, "max-b", 1, (1u << 24) - 1, false, 100);
    if ((max_a + 1) * (max_b + 1) > (1ull << 24))
        usage_error("invalid values for '--max-a' and '--max-b': (" + std::to_string(max_a) + " + 1) x (" + std::to_string(max_b) +
                    " + 1) cells is more than 16777216");
    const uint64_t mem = ranged(f, "memory", 6, 128, false, 6);
    const int threads = (int)ranged(f, "threads", 0, 1 << 20, false, 0);
    const int device = (int)ranged(f, "device", 0, 63, false, 0);
    const EstimateFlags est = estimate_flags(f);
    const bool a_table = !table_flag(f, k).empty();
    const bool b_table = !table_flag(f, k, "alt-table", "alt-input", "--alt-input <ALT_INPUT>").empty();
    if (int rc = make_out_dir(out)) return rc;
    for (const std::string &p : {a_table ? std::string() : in, b_table ? std::string() : alt}) {
        if (!p.empty() && format_from_path(p) == SeqFormat::Unknown) {  // "-" included: both inputs are read more than once
            fprintf(stderr, "Error: unsupported input extension (expected .fa/.fasta/.fna/.fq/.fastq[.gz]): %s\n", p.c_str());
            return 101;
        }
    }
    return run_table_command(est, [&]() -> std::string {
        CompareComputer cmp(in, alt, out, k);
        cmp.set_tables(a_table, b_table);
        cmp.set_max_counts((uint32_t)max_a, (uint32_t)max_b);
        if (threads > 0) cmp.set_threads(threads);
        cmp.set_max_memory((double)mem);
        cmp.set_device(device);
        return cmp.compare();
    });
}

const char *HELP_PROFILE =
    "Per-position k-mer counts and per-sequence min / median / mean / max\n\n"
    "Counts the canonical k-mers of --alt-input (default: the input) and looks up the k-mer that starts at every base of\n"
    "every input record.  Writes {output}/profile.stats: a header line, then one line per record in input order with its\n"
    "name (the header up to the first white space), length, k-mers, k-mers present in the table, min, median, mean and max\n"
    "count, tab-separated; the median is element n/2 of the n sorted counts (the upper one of an even number), the mean\n"
    "has six decimals, a record without a k-mer has zeros.  With --positions also {output}/profile.counts: per record\n"
    "\">name\" and one line of `length` space-separated counts, -1 where no k-mer starts (the last k-1 bases, windows over\n"
    "a non-ACGT base).  When the table does not fit the device memory it is counted in several passes; the per-base counts\n"
    "of the whole input (4 bytes per base) are then kept in host memory across the passes and the statistics are taken\n"
    "after the last one - refused when that array is larger than --memory.\n\n"
    "Usage: kmertools profile [OPTIONS] --input <INPUT> --output <OUTPUT> --k-size <K_SIZE>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>          Input file path (sequences to profile)\n"
    "  -o, --output <OUTPUT>        Output directory path\n"
    "  -k, --k-size <K_SIZE>        k size for counting (1..31)\n"
    "  -a, --alt-input <ALT_INPUT>  Input file path, for k-mer counting [default: the input]\n"
    "      --positions              Also write profile.counts, the count at every base\n"
    "  -m, --memory <MEMORY>        Max memory in GB [default: 6] (the table lives in HBM; bounds the per-base counts\n"
    "                               kept across the passes of an out-of-core count)\n"
    "  -t, --threads <THREADS>      Thread count for computations 0=auto [default: 0]\n"
    "      --device <DEVICE>        GPU index [default: 0]\n"
    HELP_TABLE_ALT_INPUT
    HELP_ESTIMATE
    "  -h, --help                   Print help\n";

int cmd_profile(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true},     {'o', "output", true},  {'k', "k-size", true},
                                     {'a', "alt-input", true}, {0, "positions", false}, {'m', "memory", true},
                                     {'t', "threads", true},   {0, "device", true}, SPEC_TABLE, SPEC_ESTIMATE_SIZE, SPEC_ESTIMATE_P};
    const auto f = parse_flags(argc, argv, from, specs, HELP_PROFILE);
    const std::string in = required_str(f, "input"), out = required_str(f, "output");
    const int k = (int)ranged(f, "k-size", 1, 31, true, 0);
    // everything is checked before any device work and before the output directory is made
    const uint64_t mem = ranged(f, "memory", 6, 128, false, 6);
    const int threads = (int)ranged(f, "threads", 0, 1 << 20, false, 0);
    const int device = (int)ranged(f, "device", 0, 63, false, 0);
    const EstimateFlags est = estimate_flags(f);
    const std::string table = table_flag(f, k, "table", "alt-input", "--alt-input <ALT_INPUT>");
    const std::string kin = !table.empty() ? table : f.count("alt-input") ? f.at("alt-input") : in;
    for (const std::string &p : table.empty() ? std::vector<std::string>{in, kin} : std::vector<std::string>{in}) {
        if (format_from_path(p) == SeqFormat::Unknown) {  // "-" included: both inputs are read more than once
            fprintf(stderr, "Error: unsupported input extension (expected .fa/.fasta/.fna/.fq/.fastq[.gz]): %s\n", p.c_str());
            return 101;
        }
    }
    if (int rc = make_out_dir(out)) return rc;
    return run_table_command(est, [&]() -> std::string {
        ProfileComputer prof(in, out, k);
        if (threads > 0) prof.set_threads(threads);
        if (!table.empty()) prof.set_kmer_table(table);
        else prof.set_kmer_path(kin);
        prof.set_positions(f.count("positions") != 0);
        prof.set_max_memory((double)mem);
        prof.set_device(device);
        return prof.profile();
    });
}

const char *HELP_SKETCH =
    "MinHash sketches of sequences and the Mash distances between them; scaled sketches, containment and ANI\n\n"
    "A record's sketch is the --sketch-size smallest distinct hashes of its canonical k-mers (windows over a non-ACGT base\n"
    "are none), hash = splitmix64 finaliser of (k-mer xor --seed).  Writes {output}/sketch.tsv: one line per record in input\n"
    "order with its name (the header up to the first white space), length, k-mers, sketch size and the hashes, decimal,\n"
    "ascending, comma-separated (empty at size 0), tab-separated.  With --single one sketch of the whole input: its name is\n"
    "the input's file name, its length the total number of bases.  With --alt-input the second input's sketches go to\n"
    "{output}/sketch.alt.tsv.  With --dist also {output}/sketch.dist, one line \"id_a<TAB>id_b<TAB>shared/denom<TAB>jaccard<TAB>distance\"\n"
    "per pair: the pairs i < j of the input, or every pair (record of the input, record of the alt input); denom = min(sketch\n"
    "size, hashes of the union), shared = those of the denom smallest of the union that both hold, jaccard = shared / denom,\n"
    "distance = 1 when nothing is shared, else min(1, -ln(2j / (1 + j)) / k) (Mash).\n"
    "With --scaled a sketch is instead EVERY distinct hash at or below (2^64 - 1) / N (FracMinHash: its size follows the\n"
    "content, and shared / size estimates containment whatever the two sizes); the files keep their columns, size being the\n"
    "number of hashes, and --abund adds a sixth column: how often each hash's k-mer occurred, comma-separated, parallel to\n"
    "the hashes.  With --table the one sketch is that of a table file's k-mers whose count lies in --min-count..--max-count\n"
    "(--min-count 2: the solid k-mers of a read set), the counts being the abundances: its name is the file's name, its\n"
    "length 0, its k-mers the occurrences in the count range.  With --contain also {output}/sketch.contain, one line\n"
    "\"id_a<TAB>id_b<TAB>shared<TAB>size_a<TAB>size_b<TAB>jaccard<TAB>a_in_b<TAB>b_in_a<TAB>ani\" per pair (the same pairs as sketch.dist):\n"
    "jaccard = shared / (size_a + size_b - shared), a_in_b = shared / size_a, b_in_a = shared / size_b (0 for an empty\n"
    "sketch), ani = the larger of the two containments to the power 1 / k.\n\n"
    "Usage: kmertools sketch [OPTIONS] --input <INPUT> --output <OUTPUT>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>          Input file path\n"
    "  -o, --output <OUTPUT>        Output directory path\n"
    "  -k, --k-size <K_SIZE>        k size (1..31) [default: 21]\n"
    "  -s, --sketch-size <S>        Hashes per sketch (1..16384) [default: 1000]\n"
    "      --scaled <N>             Scaled sketches: keep the hashes <= (2^64 - 1) / N (N >= 1); not with --sketch-size\n"
    "      --abund                  With --scaled: a sixth column, the abundances of the hashes\n"
    "      --seed <SEED>            Hash seed [default: 0]\n"
    "      --single                 One sketch for the whole input\n"
    "  -a, --alt-input <ALT_INPUT>  Second input: its sketches, and the distances input x alt input\n"
    "      --table <FILE>           With --scaled: sketch the k-mers of this table file (ctr --save-table) instead of\n"
    "                               --input, which is then not given; --k-size must be the file's k\n"
    "      --min-count <L>          With --table: k-mers with at least L occurrences [default: 1]\n"
    "      --max-count <U>          With --table: k-mers with at most U occurrences [default: 4294967295]\n"
    "      --dist                   Also write sketch.dist\n"
    "      --max-dist <D>           Keep the lines of sketch.dist with distance <= D (0..1) [default: 1]\n"
    "      --contain                With --scaled: also write sketch.contain\n"
    "      --min-contain <C>        Keep the lines of sketch.contain whose larger containment is >= C (0..1) [default: 0]\n"
    "  -t, --threads <THREADS>      Thread count for computations 0=auto [default: 0]\n"
    "      --device <DEVICE>        GPU index [default: 0]\n"
    "  -h, --help                   Print help\n";

// a flag's value as a number in 0..=1
static double unit_value(const std::string &v, const char *flag) {
    char *end = nullptr;
    const double x = strtod(v.c_str(), &end);
    if (v.empty() || *end || !(x >= 0.0 && x <= 1.0)) usage_error("invalid value '" + v + "' for '--" + flag + "': not a number in 0..=1");
    return x;
}

int cmd_sketch(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true},   {'o', "output", true},    {'k', "k-size", true}, {'s', "sketch-size", true},
                                     {0, "seed", true},      {0, "single", false},     {'a', "alt-input", true}, {0, "dist", false},
                                     {0, "max-dist", true},  {'t', "threads", true},   {0, "device", true},   {0, "scaled", true},
                                     {0, "abund", false},    SPEC_TABLE,               {0, "min-count", true}, {0, "max-count", true},
                                     {0, "contain", false},  {0, "min-contain", true}};
    const auto f = parse_flags(argc, argv, from, specs, HELP_SKETCH);
    const bool has_table = f.count("table") != 0;
    const std::string in = has_table && !f.count("input") ? "" : required_str(f, "input"), out = required_str(f, "output");
    // everything is checked before any device work and before the output directory is made
    const int k = (int)ranged(f, "k-size", 1, 31, false, 21);
    const uint32_t s = (uint32_t)ranged(f, "sketch-size", 1, KT_SKETCH_MAX_S, false, 1000);
    const uint64_t seed = ranged(f, "seed", 0, UINT64_MAX, false, 0);
    const int threads = (int)ranged(f, "threads", 0, 1 << 20, false, 0);
    const int device = (int)ranged(f, "device", 0, 63, false, 0);
    bool is_scaled = false;
    const uint64_t scaled = ranged(f, "scaled", 1, UINT64_MAX, false, 0, &is_scaled);
    if (is_scaled && f.at("scaled")[0] == '-')  // (strtoull takes a sign and wraps)
        usage_error("invalid value '" + f.at("scaled") + "' for '--scaled': invalid digit found in string");
    const bool dist = f.count("dist") != 0, contain = f.count("contain") != 0;
    if (is_scaled) {
        if (f.count("sketch-size")) usage_error("the argument '--scaled <N>' cannot be used with '--sketch-size <S>'");
        if (dist) usage_error("the argument '--dist' cannot be used with '--scaled <N>' (scaled sketches are compared by '--contain')");
        if (f.count("max-dist")) usage_error("the argument '--max-dist <D>' cannot be used with '--scaled <N>'");
    } else {
        for (const char *flag : {"abund", "contain", "min-contain", "table"})
            if (f.count(flag)) usage_error(std::string("the argument '--") + flag + "' requires '--scaled <N>'");
    }
    for (const char *flag : {"min-count", "max-count"})
        if (f.count(flag) && !has_table) usage_error(std::string("the argument '--") + flag + "' requires '--table <FILE>'");
    const uint32_t min_count = (uint32_t)ranged(f, "min-count", 1, 0xFFFFFFFFull, false, 1);
    const uint32_t max_count = (uint32_t)ranged(f, "max-count", 1, 0xFFFFFFFFull, false, 0xFFFFFFFFull);
    if (min_count > max_count) usage_error("'--min-count <L>' is above '--max-count <U>'");
    double max_dist = 1.0, min_contain = 0.0;
    if (auto it = f.find("max-dist"); it != f.end()) {
        if (!dist) usage_error("the argument '--max-dist <D>' requires '--dist'");
        max_dist = unit_value(it->second, "max-dist");
    }
    if (auto it = f.find("min-contain"); it != f.end()) {
        if (!contain) usage_error("the argument '--min-contain <C>' requires '--contain'");
        min_contain = unit_value(it->second, "min-contain");
    }
    const std::string table = table_flag(f, k);
    const std::string alt = f.count("alt-input") ? f.at("alt-input") : "";
    for (const std::string &p : {in, alt}) {
        if (!p.empty() && format_from_path(p) == SeqFormat::Unknown) {
            fprintf(stderr, "Error: unsupported input extension (expected .fa/.fasta/.fna/.fq/.fastq[.gz]): %s\n", p.c_str());
            return 101;
        }
    }
    if (int rc = make_out_dir(out)) return rc;
    SketchComputer sk(in, out, k, s);
    sk.set_seed(seed);
    sk.set_single(f.count("single") != 0);
    sk.set_alt_path(alt);
    sk.set_dist(dist, max_dist);
    if (is_scaled) {
        sk.set_scaled(scaled, f.count("abund") != 0);
        sk.set_table(table, min_count, max_count);
        sk.set_contain(contain, min_contain);
    }
    if (threads > 0) sk.set_threads(threads);
    sk.set_device(device);
    if (std::string e = sk.sketch(); !e.empty()) {
        fprintf(stderr, "Error: %s\n", e.c_str());
        return 101;
    }
    return 0;
}

const char *HELP_CARD =
    "Estimate the number of distinct k-mers (HyperLogLog), sizes tables\n\n"
    "One walk over the input: every canonical k-mer (windows over a non-ACGT base are none) is hashed, hash = splitmix64\n"
    "finaliser of (k-mer xor --seed); its top --precision bits pick one of 2^precision registers, which keeps the largest\n"
    "rank (1 + leading zeros of the other bits) it has seen.  Writes {output}/card.stats, one \"name<TAB>value\" line each:\n"
    "sequences, bases, kmers, precision, registers, zero_registers, distinct_estimate (Ertl's improved estimator, rounded),\n"
    "rel_std_error (1.04 / sqrt(registers), six decimals) and slots_wanted (the table --estimate-size would ask for: 1.9 slots\n"
    "for the estimate plus five standard errors, never more than the input's size allows), and {output}/card.registers: the\n"
    "line \"precision<TAB>seed<TAB>k\", then one register per line - registers of the same three numbers merge by taking the\n"
    "larger of every pair.  With --alt-input the second input's rows follow with an alt_ prefix, then union_estimate (from\n"
    "the merged registers), intersection_estimate (the two estimates minus the union's, at least 0) and jaccard_estimate (six\n"
    "decimals, 0 when the union is 0); its registers go to {output}/card.alt.registers.\n\n"
    "Usage: kmertools card [OPTIONS] --input <INPUT> --output <OUTPUT> --k-size <K_SIZE>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>          Input file path\n"
    "  -o, --output <OUTPUT>        Output directory path\n"
    "  -k, --k-size <K_SIZE>        k size (1..31)\n"
    "  -p, --precision <P>          2^P registers (4..16) [default: 14]\n"
    "      --seed <SEED>            Hash seed [default: 0]\n"
    "  -a, --alt-input <ALT_INPUT>  Second input: its estimate, and the union, intersection and Jaccard estimates\n"
    "  -t, --threads <THREADS>      Thread count for computations 0=auto [default: 0]\n"
    "      --device <DEVICE>        GPU index [default: 0]\n"
    "  -h, --help                   Print help\n";

int cmd_card(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true}, {'o', "output", true},    {'k', "k-size", true},  {'p', "precision", true},
                                     {0, "seed", true},    {'a', "alt-input", true}, {'t', "threads", true}, {0, "device", true}};
    const auto f = parse_flags(argc, argv, from, specs, HELP_CARD);
    const std::string in = required_str(f, "input"), out = required_str(f, "output");
    // everything is checked before any device work and before the output directory is made
    const int k = (int)ranged(f, "k-size", 1, 31, true, 0);
    const int p = (int)ranged(f, "precision", KT_CARD_MIN_P, KT_CARD_MAX_P, false, 14);
    const uint64_t seed = ranged(f, "seed", 0, UINT64_MAX, false, 0);
    const int threads = (int)ranged(f, "threads", 0, 1 << 20, false, 0);
    const int device = (int)ranged(f, "device", 0, 63, false, 0);
    const std::string alt = f.count("alt-input") ? f.at("alt-input") : "";
    for (const std::string &path : f.count("alt-input") ? std::vector<std::string>{in, alt} : std::vector<std::string>{in}) {
        if (format_from_path(path) == SeqFormat::Unknown) {  // "-" included: the sizing looks at the file
            fprintf(stderr, "Error: unsupported input extension (expected .fa/.fasta/.fna/.fq/.fastq[.gz]): %s\n", path.c_str());
            return 101;
        }
    }
    if (int rc = make_out_dir(out)) return rc;
    CardComputer card(in, out, k, p);
    card.set_seed(seed);
    card.set_alt_path(alt);
    if (threads > 0) card.set_threads(threads);
    card.set_device(device);
    if (std::string e = card.card(); !e.empty()) {
        fprintf(stderr, "Error: %s\n", e.c_str());
        return 101;
    }
    return 0;
}

const char *HELP_SETOP =
    "Intersect, subtract, union or xor the k-mer sets of two inputs\n\n"
    "Counts the canonical k-mers of both inputs.  A k-mer is in the input when min-a <= its count there <= max-a, in the alt\n"
    "input when min-b <= its count there <= max-b (an absent k-mer is in neither; a count outside its range is taken as 0).\n"
    "Writes the k-mers for which --op holds to {output}/kmers.counts, one \"kmer<TAB>count\" line each as `ctr` writes them,\n"
    "in ascending order of the numeric k-mer (with --acgt too; when the tables do not fit the device memory they are\n"
    "counted in several passes and each pass's lines are in that order, the passes one after the other), and\n"
    "{output}/setop.stats: distinct_a, distinct_b, in_a, in_b, emitted and emitted_occurrences, one \"name<TAB>value\" line each.\n\n"
    "Usage: kmertools setop [OPTIONS] --input <INPUT> --alt-input <ALT_INPUT> --output <OUTPUT> --k-size <K_SIZE> --op <OP>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>          Input file path (A)\n"
    "  -a, --alt-input <ALT_INPUT>  Input file path (B)\n"
    "  -o, --output <OUTPUT>        Output directory path\n"
    "  -k, --k-size <K_SIZE>        k size for counting\n"
    "      --op <OP>                Which k-mers to write [possible values: intersect, subtract, union, xor]\n"
    "                               (in A and B; in A, not in B; in A or B; in exactly one)\n"
    "      --count <COUNT>          The count to write, from the in-range counts a and b [default: first]\n"
    "                               [possible values: first, min, max, sum] (first: a, else b; min / max of the non-zero\n"
    "                               ones; sum saturates at 4294967295)\n"
    "      --min-a <N>              Lowest count of a k-mer of A [default: 1]\n"
    "      --max-a <N>              Highest count of a k-mer of A [default: 4294967295]\n"
    "      --min-b <N>              Lowest count of a k-mer of B [default: 1]\n"
    "      --max-b <N>              Highest count of a k-mer of B [default: 4294967295]\n"
    "      --acgt                   Output ACGT instead of numeric values\n"
    "  -m, --memory <MEMORY>        Max memory in GB [default: 6] (the tables live in HBM: when both and the result cannot\n"
    "                               fit, the inputs are counted in several passes; the text is written in slabs)\n"
    "  -t, --threads <THREADS>      Thread count for computations 0=auto [default: 0]\n"
    "      --device <DEVICE>        GPU index [default: 0]\n"
    HELP_TABLES
    HELP_ESTIMATE
    "  -h, --help                   Print help\n";

// the index of flag `name`'s value among `values` (clap's possible values)
int one_of(const std::map<std::string, std::string> &f, const char *name, const std::vector<std::string> &values, bool required,
           int dflt) {
    auto it = f.find(name);
    if (it == f.end()) {
        if (required) usage_error(std::string("the following required arguments were not provided:\n  --") + name);
        return dflt;
    }
    std::string all;
    for (size_t i = 0; i < values.size(); i++) {
        if (it->second == values[i]) return (int)i;
        all += (i ? ", " : "") + values[i];
    }
    usage_error("invalid value '" + it->second + "' for '--" + name + "'\n  [possible values: " + all + "]");
}

int cmd_setop(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true},  {'a', "alt-input", true}, {'o', "output", true}, {'k', "k-size", true},
                                     {0, "op", true},       {0, "count", true},       {0, "min-a", true},    {0, "max-a", true},
                                     {0, "min-b", true},    {0, "max-b", true},       {0, "acgt", false},    {'m', "memory", true},
                                     {'t', "threads", true}, {0, "device", true}, SPEC_TABLE, SPEC_ALT_TABLE, SPEC_ESTIMATE_SIZE, SPEC_ESTIMATE_P};
    const auto f = parse_flags(argc, argv, from, specs, HELP_SETOP);
    // (--table FILE stands in for --input, --alt-table FILE for --alt-input)
    const std::string in = f.count("table") ? f.at("table") : required_str(f, "input");
    const std::string alt = f.count("alt-table") ? f.at("alt-table") : required_str(f, "alt-input"), out = required_str(f, "output");
    const int k = (int)ranged(f, "k-size", 10, 31, true, 0);
    // everything is checked before any device work and before the output directory is made
    static_assert(KT_SET_INTERSECT == 0 && KT_SET_SUBTRACT == 1 && KT_SET_UNION == 2 && KT_SET_XOR == 3, "the order of --op's values");
    static_assert(KT_SETCNT_FIRST == 0 && KT_SETCNT_MIN == 1 && KT_SETCNT_MAX == 2 && KT_SETCNT_SUM == 3, "... and of --count's");
    const int op = one_of(f, "op", {"intersect", "subtract", "union", "xor"}, true, 0);     // = KT_SET_*
    const int rule = one_of(f, "count", {"first", "min", "max", "sum"}, false, 0);          // = KT_SETCNT_*
    uint64_t lo[2], hi[2];
    for (int j = 0; j < 2; j++) {
        const std::string mn = j ? "min-b" : "min-a", mx = j ? "max-b" : "max-a";
        lo[j] = ranged(f, mn.c_str(), 1, 0xFFFFFFFFull, false, 1);
        hi[j] = ranged(f, mx.c_str(), 1, 0xFFFFFFFFull, false, 0xFFFFFFFFull);
        if (lo[j] > hi[j])
            usage_error("invalid values for '--" + mn + "' and '--" + mx + "': " + std::to_string(lo[j]) + " is greater than " +
                        std::to_string(hi[j]));
    }
    const uint64_t mem = ranged(f, "memory", 6, 128, false, 6);
    const int threads = (int)ranged(f, "threads", 0, 1 << 20, false, 0);
    const int device = (int)ranged(f, "device", 0, 63, false, 0);
    const EstimateFlags est = estimate_flags(f);
    const bool a_table = !table_flag(f, k).empty();
    const bool b_table = !table_flag(f, k, "alt-table", "alt-input", "--alt-input <ALT_INPUT>").empty();
    for (const std::string &p : {a_table ? std::string() : in, b_table ? std::string() : alt}) {
        if (!p.empty() && format_from_path(p) == SeqFormat::Unknown) {  // "-" included: both inputs are read more than once
            fprintf(stderr, "Error: unsupported input extension (expected .fa/.fasta/.fna/.fq/.fastq[.gz]): %s\n", p.c_str());
            return 101;
        }
    }
    if (int rc = make_out_dir(out)) return rc;
    return run_table_command(est, [&]() -> std::string {
        SetopComputer so(in, alt, out, k);
        so.set_tables(a_table, b_table);
        so.set_op(op, rule);
        so.set_ranges((uint32_t)lo[0], (uint32_t)hi[0], (uint32_t)lo[1], (uint32_t)hi[1]);
        so.set_acgt_output(f.count("acgt") != 0);
        if (threads > 0) so.set_threads(threads);
        so.set_max_memory((double)mem);
        so.set_device(device);
        return so.setop();
    });
}

const char *HELP_GRAPH =
    "De Bruijn adjacency, unitig ends and node census of the counted k-mers\n\n"
    "Counts the canonical k-mers of the input.  A k-mer is a node when min-count <= its count <= max-count.  Writes one line\n"
    "per node to {output}/graph.nodes, in ascending order of the numeric k-mer (with --acgt too):\n"
    "\"kmer<TAB>count<TAB>left4<TAB>right4<TAB>ends2\", the k-mer as `ctr` writes it.  Position x of right4 is \"ACGT\"[x] when the\n"
    "k-mer's last k - 1 bases followed by that base are a node (either strand), of left4 when that base followed by its first\n"
    "k - 1 bases are one, else \".\"; ends2 is \"L\" or \".\" followed by \"R\" or \".\": a unitig ends at that side (the side has no\n"
    "or several neighbours, or its neighbour has several on the facing side).  {output}/graph.stats holds the census, one\n"
    "\"name<TAB>value\" line each: nodes, occurrences, degree_sum, end_sides, isolated, tips, branching and degree_<l>_<r>, the\n"
    "nodes with l left and r right neighbours (l, r = 0..4).  The whole table must fit the device memory: a k-mer's neighbours\n"
    "live anywhere in it, so graph cannot count in several passes as the other commands do, and says so before it writes.\n\n"
    "Usage: kmertools graph [OPTIONS] --input <INPUT> --output <OUTPUT> --k-size <K_SIZE>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>          Input file path\n"
    "  -o, --output <OUTPUT>        Output directory path\n"
    "  -k, --k-size <K_SIZE>        k size for counting\n"
    "      --min-count <N>          Lowest count of a node [default: 1]\n"
    "      --max-count <N>          Highest count of a node [default: 4294967295]\n"
    "      --acgt                   Output ACGT instead of numeric values\n"
    "      --stats-only             Write graph.stats only, no graph.nodes\n"
    "  -m, --memory <MEMORY>        Max memory in GB [default: 6] (the table lives in HBM; the text is written in slabs)\n"
    "  -t, --threads <THREADS>      Thread count for computations 0=auto [default: 0]\n"
    "      --device <DEVICE>        GPU index [default: 0]\n"
    HELP_TABLE
    HELP_ESTIMATE
    HELP_PREFILTER
    "  -h, --help                   Print help\n";

int cmd_graph(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true},     {'o', "output", true},      {'k', "k-size", true},  {0, "min-count", true},
                                     {0, "max-count", true},   {0, "acgt", false},         {0, "stats-only", false}, {'m', "memory", true},
                                     {'t', "threads", true},   {0, "device", true}, SPEC_TABLE, SPEC_ESTIMATE_SIZE, SPEC_ESTIMATE_P,
                                     SPEC_PREFILTER, SPEC_PREFILTER_BITS};
    const auto f = parse_flags(argc, argv, from, specs, HELP_GRAPH);
    // (--table FILE stands in for --input)
    const std::string in = f.count("table") && !f.count("input") ? "" : required_str(f, "input"), out = required_str(f, "output");
    const int k = (int)ranged(f, "k-size", 10, 31, true, 0);
    // everything is checked before any device work and before the output directory is made
    const uint64_t lo = ranged(f, "min-count", 1, 0xFFFFFFFFull, false, 1);
    const uint64_t hi = ranged(f, "max-count", 1, 0xFFFFFFFFull, false, 0xFFFFFFFFull);
    if (lo > hi)
        usage_error("invalid values for '--min-count' and '--max-count': " + std::to_string(lo) + " is greater than " + std::to_string(hi));
    const uint64_t mem = ranged(f, "memory", 6, 128, false, 6);
    const int threads = (int)ranged(f, "threads", 0, 1 << 20, false, 0);
    const int device = (int)ranged(f, "device", 0, 63, false, 0);
    const EstimateFlags est = estimate_flags(f);
    const PrefilterFlags pre = prefilter_flags(f, lo);
    const std::string table = table_flag(f, k);
    if (table.empty() && format_from_path(in) == SeqFormat::Unknown) {  // "-" included: the sizing looks at the file
        fprintf(stderr, "Error: unsupported input extension (expected .fa/.fasta/.fna/.fq/.fastq[.gz]): %s\n", in.c_str());
        return 101;
    }
    if (int rc = make_out_dir(out)) return rc;
    set_prefilter(pre.on, pre.bits, out);
    return run_table_command(est, [&]() -> std::string {
        GraphComputer gc(in, out, k);
        gc.set_table_file(table);
        gc.set_range((uint32_t)lo, (uint32_t)hi);
        gc.set_acgt_output(f.count("acgt") != 0);
        gc.set_stats_only(f.count("stats-only") != 0);
        if (threads > 0) gc.set_threads(threads);
        gc.set_max_memory((double)mem);
        gc.set_device(device);
        return gc.graph();
    });
}

const char *HELP_HETMERS =
    "Heterozygous k-mer pairs of the counted k-mers and their coverage matrix\n\n"
    "Counts the canonical k-mers of the input.  A k-mer is solid when min-count <= its count <= max-count.  Two solid k-mers\n"
    "are a pair when they differ in exactly one base (either strand) and neither has another solid k-mer at one substitution:\n"
    "the two alleles of an isolated heterozygous site (Smudgeplot's hetkmers).  Writes, in ascending order of the numeric\n"
    "smaller k-mer A of each pair:\n"
    "  {output}/hetmers.pairs   \"A<TAB>B<TAB>pos<TAB>count_a<TAB>count_b\": both k-mers as letters, B on the strand on which it\n"
    "                           differs from A at the one 0-based position pos\n"
    "  {output}/hetmers.cov     \"minor<TAB>major\": the smaller and the larger of the pair's two counts, in the same order\n"
    "  {output}/hetmers.matrix  line r (r = 0..max-minor) holds max-major + 1 tab-separated numbers: the pairs whose minor\n"
    "                           count is r and whose major count is the column; the last row and column count theirs or more\n"
    "  {output}/hetmers.stats   one \"name<TAB>value\" line each: k, min_count, max_count, positions (all or middle), nodes,\n"
    "                           occurrences, degree_0, degree_1, degree_2_or_more (solid k-mers with that many solid k-mers\n"
    "                           at one substitution), pairs, minor_sum, major_sum\n"
    "The whole table must fit the device memory, as for `graph`: a k-mer's partners live anywhere in it, so hetmers cannot\n"
    "count in several passes, and says so before it writes.\n\n"
    "Usage: kmertools hetmers [OPTIONS] --input <INPUT> --output <OUTPUT> --k-size <K_SIZE>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>          Input file path\n"
    "  -o, --output <OUTPUT>        Output directory path\n"
    "  -k, --k-size <K_SIZE>        k size for counting\n"
    "      --min-count <N>          Lowest count of a solid k-mer [default: 1]\n"
    "      --max-count <N>          Highest count of a solid k-mer [default: 4294967295]\n"
    "      --middle                 Substitutions of the middle base only (odd k)\n"
    "      --max-minor <N>          Highest minor count of the rows; the last row counts N or more [default: 500]\n"
    "      --max-major <N>          Highest major count of the columns; the last column counts N or more [default: 1000]\n"
    "      --stats-only             Write hetmers.matrix and hetmers.stats only, no hetmers.pairs and hetmers.cov\n"
    "  -m, --memory <MEMORY>        Max memory in GB [default: 6] (accepted as for graph; the table lives in HBM)\n"
    "  -t, --threads <THREADS>      Thread count for computations 0=auto [default: 0]\n"
    "      --device <DEVICE>        GPU index [default: 0]\n"
    HELP_TABLE
    HELP_ESTIMATE
    HELP_PREFILTER
    "  -h, --help                   Print help\n";

int cmd_hetmers(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true},   {'o', "output", true},    {'k', "k-size", true},    {0, "min-count", true},
                                     {0, "max-count", true}, {0, "middle", false},     {0, "max-minor", true},   {0, "max-major", true},
                                     {0, "stats-only", false}, {'m', "memory", true},  {'t', "threads", true},   {0, "device", true},
                                     SPEC_TABLE, SPEC_ESTIMATE_SIZE, SPEC_ESTIMATE_P, SPEC_PREFILTER, SPEC_PREFILTER_BITS};
    const auto f = parse_flags(argc, argv, from, specs, HELP_HETMERS);
    // (--table FILE stands in for --input)
    const std::string in = f.count("table") && !f.count("input") ? "" : required_str(f, "input"), out = required_str(f, "output");
    const int k = (int)ranged(f, "k-size", 10, 31, true, 0);
    // everything is checked before any device work and before the output directory is made
    const uint64_t lo = ranged(f, "min-count", 1, 0xFFFFFFFFull, false, 1);
    const uint64_t hi = ranged(f, "max-count", 1, 0xFFFFFFFFull, false, 0xFFFFFFFFull);
    if (lo > hi)
        usage_error("invalid values for '--min-count' and '--max-count': " + std::to_string(lo) + " is greater than " + std::to_string(hi));
    const bool middle = f.count("middle") != 0;
    if (middle && k % 2 == 0)
        usage_error("invalid value '" + std::to_string(k) + "' for '--k-size <K_SIZE>' with '--middle': an even k has no middle base");
    const uint64_t max_minor = ranged(f, "max-minor", 1, (1u << 24) - 1, false, 500);
    const uint64_t max_major = ranged(f, "max-major", 1, (1u << 24) - 1, false, 1000);
    if ((max_minor + 1) * (max_major + 1) > (1ull << 24))
        usage_error("invalid values for '--max-minor' and '--max-major': (" + std::to_string(max_minor) + " + 1) x (" +
                    std::to_string(max_major) + " + 1) cells is more than 16777216");
    const uint64_t mem = ranged(f, "memory", 6, 128, false, 6);
    const int threads = (int)ranged(f, "threads", 0, 1 << 20, false, 0);
    const int device = (int)ranged(f, "device", 0, 63, false, 0);
    const EstimateFlags est = estimate_flags(f);
    const PrefilterFlags pre = prefilter_flags(f, lo);
    const std::string table = table_flag(f, k);
    if (table.empty() && format_from_path(in) == SeqFormat::Unknown) {  // "-" included: the sizing looks at the file
        fprintf(stderr, "Error: unsupported input extension (expected .fa/.fasta/.fna/.fq/.fastq[.gz]): %s\n", in.c_str());
        return 101;
    }
    if (int rc = make_out_dir(out)) return rc;
    set_prefilter(pre.on, pre.bits, out);
    return run_table_command(est, [&]() -> std::string {
        HetmerComputer hc(in, out, k);
        hc.set_table_file(table);
        hc.set_range((uint32_t)lo, (uint32_t)hi);
        hc.set_middle(middle);
        hc.set_max_counts((uint32_t)max_minor, (uint32_t)max_major);
        hc.set_stats_only(f.count("stats-only") != 0);
        if (threads > 0) hc.set_threads(threads);
        hc.set_max_memory((double)mem);
        hc.set_device(device);
        return hc.hetmers();
    });
}

const char *HELP_UNITIGS =
    "Maximal unitigs of the de Bruijn graph of the counted k-mers\n\n"
    "Counts the canonical k-mers of the input.  A k-mer is a node when min-count <= its count <= max-count; nodes are chained\n"
    "through the sides at which `graph` reports no unitig end (a k-mer that follows itself, a hairpin and a k-mer that is its\n"
    "own reverse complement end a chain as well).  Every chain is one unitig of nodes + k - 1 bases: a path is written from its\n"
    "end with the smaller canonical k-mer, a cycle from its smallest canonical k-mer, once around.  {output}/unitigs.fa holds, in\n"
    "ascending order of that first k-mer, \">{i} LN:i:{bases} KC:i:{sum of the k-mers' counts} km:f:{that sum / k-mers}\" (and\n"
    "\" CL:i:1\" on a cycle), then the sequence on one line.  {output}/unitigs.stats holds one \"name<TAB>value\" line each:\n"
    "unitigs, bases, nodes, occurrences, circular, singletons, longest, n50.  The whole table must fit the device memory, as\n"
    "for `graph`: unitigs cannot count in several passes, and says so before it writes.\n\n"
    "The edges of the compacted graph: unitig u read as written is (u, +), its reverse complement (u, -); (u, su) links to\n"
    "(v, sv) when the last k - 1 bases of the one are the first k - 1 of the other (u = v included; every link has a mirror\n"
    "(v, !sv) -> (u, !su)).  --links appends \" L:{su}:{v}:{sv}\" for every link of the unitig to its header line in unitigs.fa\n"
    "(BCALM's form).  --gfa writes {output}/unitigs.gfa: \"H<TAB>VN:Z:1.0\", one\n"
    "\"S<TAB>{i}<TAB>{sequence}<TAB>LN:i:<TAB>KC:i:<TAB>km:f:\" line per unitig (and \"<TAB>CL:i:1\" on a cycle) and one\n"
    "\"L<TAB>{u}<TAB>{su}<TAB>{v}<TAB>{sv}<TAB>{k-1}M\" line per link, a link and its mirror written once.  Either flag also\n"
    "writes {output}/unitigs.links.stats: links, edges (L lines), dead_ends, isolated, self_links, max_end_degree.\n\n"
    "--clip-tips cleans the graph before anything is written, so that every file describes the clipped graph.  A unitig of at\n"
    "most --tip-nodes k-mers that is no cycle and has links at one end only is a tip when every end it links to has another\n"
    "link to a unitig that is no such dead end, or is one with a higher mean count (then: a lower number).  The tips' k-mers are\n"
    "erased from the table and the unitigs made again, for --clip-rounds rounds or until a round finds no tip;\n"
    "--drop-isolated erases the unitigs that short without a link at either end as well.  {output}/unitigs.clip.stats holds\n"
    "rounds, tips, tip_nodes, isolated, isolated_nodes, occurrences (all erased) and converged (1: the last round found\n"
    "nothing, 0: stopped by --clip-rounds).\n\n"
    "--pop-bubbles removes the short parallel paths that a SNP, a small indel or a repeated error leaves: of the unitigs of at\n"
    "most --bubble-nodes k-mers that are no cycles and have exactly one link at either end, to the same two ends of other\n"
    "unitigs, only the one with the highest mean count (then: the lowest number) stays.  The others' k-mers are erased and the\n"
    "unitigs made again, for --clip-rounds rounds or until a round finds nothing; with --clip-tips both rules mark the unitigs\n"
    "of every round, so that a bubble behind a tip pops in the round after the tip went.  {output}/unitigs.simplify.stats then\n"
    "holds rounds, tips, tip_nodes, isolated, isolated_nodes, popped, popped_nodes, bubbles, occurrences (all erased) and\n"
    "converged, and takes the place of unitigs.clip.stats.\n\n"
    "--components finds the connected components of the graph that is written (after --clip-tips / --pop-bubbles): two unitigs\n"
    "are in one component when a chain of links, followed in either direction, joins them.  Components are numbered by their\n"
    "smallest unitig.  {output}/unitigs.components holds one line per component:\n"
    "component<TAB>unitigs<TAB>nodes<TAB>bases<TAB>count_sum<TAB>km<TAB>links<TAB>first_unitig (bases = nodes + (k - 1) * unitigs,\n"
    "km = count_sum / nodes, links = the directed links its unitigs' ends own); {output}/unitigs.components.stats holds\n"
    "components, singletons (components of one unitig), largest_unitigs, largest_nodes and largest_share (largest_nodes / nodes);\n"
    "unitigs.links.stats is written as with --gfa.  Unless --stats-only is given, every header line of unitigs.fa gains\n"
    "\" CC:i:{component}\" and every S line of unitigs.gfa \"<TAB>CC:i:{component}\", behind the other fields.\n\n"
    "Usage: kmertools unitigs [OPTIONS] --input <INPUT> --output <OUTPUT> --k-size <K_SIZE>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>          Input file path\n"
    "  -o, --output <OUTPUT>        Output directory path\n"
    "  -k, --k-size <K_SIZE>        k size for counting\n"
    "      --min-count <N>          Lowest count of a node [default: 1]\n"
    "      --max-count <N>          Highest count of a node [default: 4294967295]\n"
    "      --stats-only             Write unitigs.stats only, no unitigs.fa\n"
    "      --gfa                    Also write unitigs.gfa (S and L lines) and unitigs.links.stats\n"
    "      --links                  Append L:{su}:{v}:{sv} fields to the header lines of unitigs.fa; also unitigs.links.stats\n"
    "      --clip-tips              Erase the tips from the table before the unitigs are written; also unitigs.clip.stats\n"
    "      --tip-nodes <N>          Longest tip, in k-mers [default: k] (needs --clip-tips)\n"
    "      --clip-rounds <R>        Most rounds of clipping, 1..1024 [default: 8] (needs --clip-tips or --pop-bubbles)\n"
    "      --drop-isolated          Erase the isolated unitigs of at most --tip-nodes k-mers too (needs --clip-tips)\n"
    "      --pop-bubbles            Erase all but the best of parallel branches before the unitigs are written; also\n"
    "                               unitigs.simplify.stats\n"
    "      --bubble-nodes <N>       Longest branch of a bubble, in k-mers [default: 2k] (needs --pop-bubbles)\n"
    "      --components             Also write unitigs.components, unitigs.components.stats and unitigs.links.stats; CC:i: fields\n"
    "                               in unitigs.fa and unitigs.gfa (allowed with --stats-only)\n"
    "  -m, --memory <MEMORY>        Max memory in GB [default: 6] (accepted as for graph; the table lives in HBM)\n"
    "  -t, --threads <THREADS>      Thread count for computations 0=auto [default: 0] (accepted as for graph)\n"
    "      --device <DEVICE>        GPU index [default: 0]\n"
    HELP_TABLE
    HELP_ESTIMATE
    HELP_PREFILTER
    "  -h, --help                   Print help\n";

int cmd_unitigs(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true},     {'o', "output", true},      {'k', "k-size", true},  {0, "min-count", true},
                                     {0, "max-count", true},   {0, "stats-only", false},   {'m', "memory", true},  {'t', "threads", true},
                                     {0, "device", true},      {0, "gfa", false},          {0, "links", false},
                                     {0, "clip-tips", false},  {0, "tip-nodes", true},     {0, "clip-rounds", true},
                                     {0, "drop-isolated", false}, {0, "pop-bubbles", false}, {0, "bubble-nodes", true}, {0, "components", false}, SPEC_TABLE, SPEC_ESTIMATE_SIZE, SPEC_ESTIMATE_P,
                                     SPEC_PREFILTER, SPEC_PREFILTER_BITS};
    const auto f = parse_flags(argc, argv, from, specs, HELP_UNITIGS);
    // (--table FILE stands in for --input)
    const std::string in = f.count("table") && !f.count("input") ? "" : required_str(f, "input"), out = required_str(f, "output");
    const int k = (int)ranged(f, "k-size", 10, 31, true, 0);
    // everything is checked before any device work and before the output directory is made
    const uint64_t lo = ranged(f, "min-count", 1, 0xFFFFFFFFull, false, 1);
    const uint64_t hi = ranged(f, "max-count", 1, 0xFFFFFFFFull, false, 0xFFFFFFFFull);
    if (lo > hi)
        usage_error("invalid values for '--min-count' and '--max-count': " + std::to_string(lo) + " is greater than " + std::to_string(hi));
    (void)ranged(f, "memory", 6, 128, false, 6);
    (void)ranged(f, "threads", 0, 1 << 20, false, 0);
    const int device = (int)ranged(f, "device", 0, 63, false, 0);
    const bool gfa = f.count("gfa") != 0, links = f.count("links") != 0;
    if (f.count("stats-only") && gfa) usage_error("the argument '--stats-only' cannot be used with '--gfa'");
    if (f.count("stats-only") && links) usage_error("the argument '--stats-only' cannot be used with '--links'");
    const bool clip = f.count("clip-tips") != 0;
    const uint64_t tip_nodes = ranged(f, "tip-nodes", 1, 0x7FFFFFFEull, false, (uint64_t)k);
    const uint64_t clip_rounds = ranged(f, "clip-rounds", 1, 1024, false, 8);
    const bool pop = f.count("pop-bubbles") != 0;
    const uint64_t bubble_nodes = ranged(f, "bubble-nodes", 1, 0x7FFFFFFEull, false, 2 * (uint64_t)k);
    for (const char *needs : {"tip-nodes", "clip-rounds", "drop-isolated"})
        if (f.count(needs) && !clip && !(pop && std::string(needs) == "clip-rounds"))
            usage_error(std::string("the argument '--") + needs + "' requires '--clip-tips'");
    if (f.count("bubble-nodes") && !pop) usage_error("the argument '--bubble-nodes' requires '--pop-bubbles'");
    const EstimateFlags est = estimate_flags(f);
    const PrefilterFlags pre = prefilter_flags(f, lo);
    const std::string table = table_flag(f, k);
    if (table.empty() && format_from_path(in) == SeqFormat::Unknown) {  // "-" included: the sizing looks at the file
        fprintf(stderr, "Error: unsupported input extension (expected .fa/.fasta/.fna/.fq/.fastq[.gz]): %s\n", in.c_str());
        return 101;
    }
    if (int rc = make_out_dir(out)) return rc;
    set_prefilter(pre.on, pre.bits, out);
    return run_table_command(est, [&]() -> std::string {
        UnitigComputer uc(in, out, k);
        uc.set_table_file(table);
        uc.set_links(gfa, links);
        uc.set_components(f.count("components") != 0);
        if (clip) uc.set_clip((uint32_t)tip_nodes, (uint32_t)clip_rounds, f.count("drop-isolated") != 0);
        if (pop) uc.set_bubbles((uint32_t)bubble_nodes, (uint32_t)clip_rounds);
        uc.set_range((uint32_t)lo, (uint32_t)hi);
        uc.set_stats_only(f.count("stats-only") != 0);
        uc.set_device(device);
        return uc.unitigs();
    });
}

const char *HELP_THREAD =
    "Map reads onto the unitigs of the counted k-mers (exact k-mer threading), GAF output\n\n"
    "Counts the canonical k-mers of --alt-input (or loads --table), makes the unitigs of the k-mers with min-count <= count <=\n"
    "max-count exactly as `unitigs --gfa` does, and indexes them: every k-mer of the graph lies in exactly one unitig, once.\n"
    "Every record of --input is then walked: each of its k-mers (windows over a non-ACGT base are none) is a HIT at (unitig,\n"
    "offset, orientation) or a miss.  A RUN is a maximal stretch of consecutive hits that step along one unitig in one\n"
    "orientation; a walk around a circular unitig starts a new run where it wraps.  A CHAIN is a maximal sequence of runs of one\n"
    "record in which each run starts at the read position where the one before stopped and at the first k-mer of its oriented\n"
    "unitig, the one before having ended at the last k-mer of its own - a walk through the graph without a gap.\n\n"
    "Writes to {output}:\n"
    "  unitigs.fa, unitigs.gfa  byte for byte those of `unitigs --gfa` for the same table and range: the ids below are theirs\n"
    "  thread.gaf      one line per chain, 12 tab-separated columns: 1 read id (the header up to the first white space), 2 read\n"
    "                  length, 3 qstart (the read position of the first k-mer), 4 qend (the last k-mer's position + k), 5 '+',\n"
    "                  6 the path, '>u' (as written) or '<u' (reverse complement) per run, 7 path length (the sum of the unitigs'\n"
    "                  lengths - (k - 1) * (runs - 1)), 8 start on the path, 9 end on the path (start + qend - qstart), 10 and 11\n"
    "                  qend - qstart (all bases match), 12 255.  A record without a hit has no line.\n"
    "  thread.unitigs  per unitig: id, bases, nodes (k-mers), count sum of the graph, hits, runs, hits / nodes\n"
    "  thread.stats    \"name<TAB>value\" lines: reads, bases, windows, hits, misses, runs, chains, reads_with_hit,\n"
    "                  reads_one_chain_end_to_end, unitigs_hit\n"
    "With --components the unitigs' connected components are found as `unitigs --components` finds them, and:\n"
    "  unitigs.fa, unitigs.gfa  are those of `unitigs --gfa --components` (a CC:i: field per unitig); unitigs.components as there\n"
    "  thread.reads       one line per record of --input, in input order: name<TAB>component|*<TAB>mixed<TAB>hits - the\n"
    "                     component of the record's first run (* without a run), 1 when a later run lies in another component\n"
    "                     (else 0), and the record's hits\n"
    "  thread.components  per component: component<TAB>unitigs<TAB>nodes<TAB>reads<TAB>hits (the records counted at the component\n"
    "                     of their first run, every run's hits at its own)\n"
    "  thread.stats       gains reads_with_component, reads_mixed, components_hit\n"
    "The whole table must fit the device memory, as for `unitigs`; the unitigs may hold at most 2^31 - 2 bases.\n\n"
    "Usage: kmertools thread [OPTIONS] --input <INPUT> --output <OUTPUT> --k-size <K_SIZE>\n\n"
    "Options:\n"
    "  -i, --input <INPUT>          The records to thread\n"
    "  -a, --alt-input <ALT_INPUT>  Input file path, for k-mer counting [default: the input]\n"
    "  -o, --output <OUTPUT>        Output directory path\n"
    "  -k, --k-size <K_SIZE>        k size for counting\n"
    "      --min-count <N>          Lowest count of a node [default: 1]\n"
    "      --max-count <N>          Highest count of a node [default: 4294967295]\n"
    "      --stats-only             Write thread.unitigs and thread.stats only (with --components: thread.components too)\n"
    "      --components             Split the records by the connected component of the unitigs they land in: thread.reads,\n"
    "                               thread.components, unitigs.components, CC:i: fields\n"
    "  -m, --memory <MEMORY>        Max memory in GB [default: 6] (accepted as for unitigs; the table lives in HBM)\n"
    "  -t, --threads <THREADS>      Thread count for computations 0=auto [default: 0] (accepted as for unitigs)\n"
    "      --device <DEVICE>        GPU index [default: 0]\n"
    HELP_TABLE_ALT_INPUT
    HELP_ESTIMATE
    "  -h, --help                   Print help\n";

int cmd_thread(int argc, char **argv, int from) {
    const std::vector<Spec> specs = {{'i', "input", true},     {'a', "alt-input", true}, {'o', "output", true},  {'k', "k-size", true},
                                     {0, "min-count", true},   {0, "max-count", true},   {0, "stats-only", false}, {'m', "memory", true},
                                     {'t', "threads", true},   {0, "device", true},      {0, "components", false}, SPEC_TABLE, SPEC_ESTIMATE_SIZE, SPEC_ESTIMATE_P};
    const auto f = parse_flags(argc, argv, from, specs, HELP_THREAD);
    const std::string in = required_str(f, "input"), out = required_str(f, "output");
    const int k = (int)ranged(f, "k-size", 10, 31, true, 0);
    // everything is checked before any device work and before the output directory is made
    const uint64_t lo = ranged(f, "min-count", 1, 0xFFFFFFFFull, false, 1);
    const uint64_t hi = ranged(f, "max-count", 1, 0xFFFFFFFFull, false, 0xFFFFFFFFull);
    if (lo > hi)
        usage_error("invalid values for '--min-count' and '--max-count': " + std::to_string(lo) + " is greater than " + std::to_string(hi));
    (void)ranged(f, "memory", 6, 128, false, 6);
    (void)ranged(f, "threads", 0, 1 << 20, false, 0);
    const int device = (int)ranged(f, "device", 0, 63, false, 0);
    const EstimateFlags est = estimate_flags(f);
    const std::string table = table_flag(f, k, "table", "alt-input", "--alt-input <ALT_INPUT>");
    const std::string counted = !table.empty() ? "" : f.count("alt-input") ? f.at("alt-input") : in;
    for (const std::string &p : table.empty() ? std::vector<std::string>{in, counted} : std::vector<std::string>{in}) {
        if (format_from_path(p) == SeqFormat::Unknown) {  // "-" included: the inputs are sized and read from files
            fprintf(stderr, "Error: unsupported input extension (expected .fa/.fasta/.fna/.fq/.fastq[.gz]): %s\n", p.c_str());
            return 101;
        }
    }
    if (int rc = make_out_dir(out)) return rc;
    return run_table_command(est, [&]() -> std::string {
        UnitigComputer uc(counted, out, k);
        uc.set_table_file(table);
        uc.set_range((uint32_t)lo, (uint32_t)hi);
        uc.set_thread(in, f.count("stats-only") != 0);
        uc.set_components(f.count("components") != 0);
        uc.set_device(device);
        return uc.unitigs();
    });
}

// hidden: the host side of --prefilter without a device (the sanitizer builds run it): the sizing of the two arrays over
// every exponent and at the edges of u64, the table plan's arithmetic, the stats text written through write_text_file and
// read back.  Prints "prefilter ok", or what was wrong.
int cmd_debug_prefilter(int argc, char **argv, int from) {
    if (from >= argc) return 2;
    const std::string dir = argv[from];
    int bad = 0;
    auto check = [&](bool ok, const char *what) {
        if (!ok) fprintf(stderr, "debug-prefilter: %s\n", what), bad++;
    };
    int a = -1, b = -1;
    check(prefilter_sizes(0, 16, 0, &a, &b).empty() && a == 10 && b == 10, "no k-mers: the smallest filter");
    check(prefilter_sizes(1ull << 16, 1, 0, &a, &b).empty() && a == 10 && b == 10, "2^16 bits are 2^10 words");
    check(prefilter_sizes((1ull << 16) + 1, 1, 0, &a, &b).empty() && a == 11 && b == 10, "one bit more rounds up");
    for (int e = 10; e <= 34; e++) {
        check(prefilter_sizes(1ull << e, 64, 0, &a, &b).empty() && a == e && b == std::max(10, e - 2), "a word a k-mer");
        check(prefilter_sizes((1ull << e) * 4, 16, 0, &a, &b).empty() && a == e && b == std::max(10, e - 2), "16 bits a k-mer");
    }
    check(prefilter_sizes(1ull << 36, 16, 0, &a, &b).empty() && a == 34 && b == 32, "2^40 bits are 2^34 words, the most");
    check(!prefilter_sizes((1ull << 36) + 1, 16, 0, &a, &b).empty(), "one k-mer more than 2^34 words hold is refused");
    check(!prefilter_sizes(~0ull, ~0ull, 0, &a, &b).empty(), "the largest request is refused, not wrapped");
    check(!prefilter_sizes(1000, 0, 0, &a, &b).empty(), "0 bits a k-mer is refused");
    check(!prefilter_sizes(1000, 1ull << 40, 0, &a, &b).empty(), "2^40 bits for each of 1000 k-mers is refused");
    check(prefilter_sizes(1ull << 30, 16, 1ull << 30, &a, &b).empty() && a == 25 && b == 23, "a quarter of 1 GiB free: 2^25 words");
    check(prefilter_sizes(1ull << 30, 16, 1, &a, &b).empty() && a == 10 && b == 10, "no memory to speak of: the smallest filter");
    check(prefilter_table_slots(0, 0, 10, 0, 1.0) == 1024, "an empty filter: the smallest table");
    check(prefilter_table_slots(1000000, 0, 20, 5000000, 1.0) == 1900000, "1.9 slots a promotion");
    check(prefilter_table_slots(0, 64ull << 20, 20, 1000, 1.0) == 1900, "a full filter lets every k-mer in");
    check(prefilter_table_slots(0, 32ull << 20, 20, 16000, 1.0) == 1900, "half the bits set: one k-mer in sixteen");
    check(prefilter_table_slots(1000000, 0, 20, 0, 0.01) == 19000, "the scale");
    check(prefilter_table_slots(~0ull, 0, 10, ~0ull, 4.0) == ~0ull, "beyond u64: saturated");
    check(prefilter_table_slots(5, 0, 10, 0, -1.0) == 1024, "a negative scale");
    PrefilterStats st;
    st.windows = ~0ull, st.once_words = 1ull << 34, st.twice_words = 1024, st.once_bits_set = 7, st.table_retries = 2;
    const std::string want = "windows\t18446744073709551615\nonce_words\t17179869184\ntwice_words\t1024\nonce_bits_set\t7\n"
                             "twice_bits_set\t0\npromotions\t0\ntable_slots\t0\ntable_keys\t0\ntable_retries\t2\n";
    check(prefilter_stats_text(st) == want, "the stats text");
    set_prefilter(true, 16, dir);
    check(write_prefilter_stats(st).empty(), "the stats file");
    std::string got;
    if (FILE *f = fopen((dir + "/prefilter.stats").c_str(), "rb")) {
        char buf[512];
        for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) got.append(buf, n);
        fclose(f);
    }
    check(got == want, "the stats file read back");
    unlink((dir + "/prefilter.stats").c_str());
    set_prefilter(true, 16, dir + "/no/such/dir");
    check(!write_prefilter_stats(st).empty(), "a directory that does not exist is an error");
    set_prefilter(false, 16, "");
    if (!bad) printf("prefilter ok\n");
    return bad ? 1 : 0;
}

// hidden: parse a file and print its records (CPU-only reader tests)
int cmd_debug_read(int argc, char **argv, int from) {
    if (from >= argc) return 2;
    SeqReader r;
    const bool sniff = from + 1 < argc && !strcmp(argv[from + 1], "sniff");
    if (!r.open(argv[from], sniff)) {
        fprintf(stderr, "Error: %s\n", r.error().c_str());
        return 1;
    }
    Batch b;
    uint64_t total = 0, count = 0;
    // KT_DEBUG_READ_PASSES=N: the records N times over ONE reader (rewind(): the passes of an out-of-core count); every
    // odd pass before the last is left half-way (a rewind in the middle of the stream, pieces parsed ahead and never taken)
    const int passes = getenv("KT_DEBUG_READ_PASSES") ? atoi(getenv("KT_DEBUG_READ_PASSES")) : 1;
    // KT_DEBUG_READ_RECORDS=1: whole records (keep_records) - each line also carries the header and the quality
    const bool records = getenv("KT_DEBUG_READ_RECORDS") != nullptr;
    for (int pass = 0; pass < passes; pass++) {
        if (pass && !r.rewind()) break;
        const bool cut_short = (pass & 1) && pass + 1 < passes;
        if (pass) printf("#pass\t%d\n", pass);
        total = count = 0;
        for (;;) {
            const bool more = r.next_batch(b, 64, 2, true, records);  // tiny batches: exercises batch boundaries
            for (uint64_t i = 0; i < b.n_reads(); i++) {
                printf("%llu\t%s\t", (unsigned long long)(b.first_record + i), b.ids[i].c_str());
                if (records) printf("%s\t", b.headers[i].c_str());
                fwrite(b.bases.data() + b.offsets[i], 1, b.offsets[i + 1] - b.offsets[i], stdout);
                if (records && !b.quals.empty()) {
                    printf("\t");
                    fwrite(b.quals.data() + b.offsets[i], 1, b.offsets[i + 1] - b.offsets[i], stdout);
                }
                printf("\n");
            }
            count += b.n_reads();
            total += b.bases.size();
            if (!more || (cut_short && count >= 1000)) break;
        }
        if (r.failed()) break;
    }
    if (r.failed()) {
        fprintf(stderr, "Error: %s\n", r.error().c_str());
        return 1;
    }
    printf("#records\t%llu\t%llu\n", (unsigned long long)count, (unsigned long long)total);
    uint64_t c2 = 0, t2 = 0;
    std::string err;
    if (SeqReader::seq_stats(argv[from], c2, t2, err)) printf("#seq_stats\t%llu\t%llu\n", (unsigned long long)c2, (unsigned long long)t2);
    return 0;
}

// hidden: checks the hand-written {:.6} formatter against snprintf("%.6f") (both round the exact
// binary value half-to-even) on count ratios, exact ties, and random doubles
int cmd_debug_fixed6(int argc, char **argv, int from) {
    const uint64_t n = from < argc ? strtoull(argv[from], nullptr, 10) : 1000000;
    uint64_t state = 0x9e3779b97f4a7c15ull, checked = 0, bad = 0;
    auto next = [&]() {
        state += 0x9e3779b97f4a7c15ull;
        uint64_t z = state;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    };
    auto check = [&](double x) {
        char a[FIXED6_BUF], b[FIXED6_BUF];
        const size_t la = format_fixed6(a, x);
        const int lb = snprintf(b, sizeof b, "%.6f", x);
        checked++;
        if (la != (size_t)lb || memcmp(a, b, la) != 0) {
            if (bad++ < 10) fprintf(stderr, "mismatch: %.17g -> '%.*s' vs '%s'\n", x, (int)la, a, b);
        }
    };
    const double specials[] = {0.0, 1.0, 0.5, 1e-7, 5e-7, 4.9999999999999998e-7, 5.0000000000000004e-7, 0.9999995, 0.99999949999999994,
                               1.0 / 128, 3.0 / 128, 1.0 / 64, 123456.7890125, 3999999999.9999995, 4.0e9, 1e300, -1.5, 2.5e-6, 1.5e-6,
                               0.1, 0.2, 0.3, 1.0 / 3.0, 2.0 / 3.0, 1e-300, 5e-324};
    for (double x : specials) check(x);
    for (uint64_t d = 1; d <= 1200; d++)             // every count ratio of a read with up to 1200 k-mers
        for (uint64_t c = 0; c <= d; c++) check((double)c / (double)d);
    for (int m = 1; m <= 40; m++)                     // dyadic values: the only exact ties
        for (uint64_t c = 1; c < 400; c += 2) check(ldexp((double)c, -m));
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t r = next();
        check((double)(r >> 11) * 0x1p-53);                                        // uniform [0,1)
        check((double)(r >> 11) * 0x1p-53 * pow(10.0, (double)(next() % 19) - 9));   // wide range
        check((double)(next() % 2000000001ull) / 2000000.0 + 0.00000025);          // near half-way digits
    }
    printf("checked %llu mismatches %llu\n", (unsigned long long)checked, (unsigned long long)bad);
    return bad ? 1 : 0;
}

// hidden: OutFile (outfile.hpp) through its paths, the scratch files in <dir>: a directory that does not exist, /dev/full
// with little (the failure shows at close) and with much (it shows at the write), writes after a failure, a scope left
// without close(), 9 MiB in pieces that straddle the flush threshold read back, a second close()
int cmd_debug_outfile(int argc, char **argv, int from) {
    if (from >= argc) return 2;
    const std::string dir = argv[from];
    int bad = 0;
    auto check = [&](bool ok, const char *what) {
        if (!ok) fprintf(stderr, "debug-outfile: %s\n", what), bad++;
    };
    auto slurp = [](const std::string &path) {
        std::string s;
        if (FILE *f = fopen(path.c_str(), "rb")) {
            char buf[1 << 16];
            for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) s.append(buf, n);
            fclose(f);
        }
        return s;
    };
    {
        OutFile o;
        const std::string p = dir + "/no/such/dir/x";
        check(o.open(p) == "Unable to write to file: " + p, "open in a missing directory: the message");
        check(!o.is_open() && !o.failed(), "a file that did not open is not open and has not failed");
        o.text() += "nowhere";
        check(o.write("nowhere") && o.close().empty(), "a file that did not open swallows writes and closes clean");
    }
    const std::string full = "Unable to write to file: /dev/full";
    {
        OutFile o;
        check(o.open("/dev/full").empty(), "open /dev/full");
        check(o.write("0123456789") && !o.failed(), "10 bytes to /dev/full: buffered, no failure yet");
        check(o.close() == full, "10 bytes to /dev/full: the failure at close");
        check(o.close().empty() && !o.is_open(), "a second close has nothing to report");
    }
    {
        OutFile o;
        const std::string mib((size_t)1 << 20, 'x');
        check(o.open("/dev/full").empty(), "open /dev/full again");
        check(!o.write(mib) && o.failed(), "1 MiB to /dev/full: the failure at the write");
        check(!o.write("more") && !o.write(std::vector<std::string>{"a", "b"}), "writes after a failure fail");
        o.text() += "and more";
        check(o.error() == full && o.close() == full, "1 MiB to /dev/full: the same message");
        check(o.close().empty(), "the message comes once");
    }
    {
        OutFile o;  // the buffered text alone, past the threshold: the failure shows when text() is asked for again
        check(o.open("/dev/full").empty(), "open /dev/full a third time");
        o.text().assign(OutFile::FLUSH_AT, 'y');
        check(!o.failed(), "text below its next request is not written yet");
        o.text() += "z";
        check(o.failed() && o.close() == full, "a full buffer to /dev/full: the failure at the flush");
    }
    const std::string scoped = dir + "/outfile.scoped";
    {
        OutFile o;
        check(o.open(scoped).empty(), "open a file to leave open");
        o.text() += "left ";
        o.write("open");
        o.text() += "\n";
    }
    check(slurp(scoped) == "left open\n", "a scope left without close(): the destructor wrote and closed");
    {
        // 9 MiB: lines through text(), now and then a vector of pieces or a string straight through write(), in sizes
        // that put the buffer just below, at and above the threshold
        const std::string path = dir + "/outfile.big";
        OutFile o;
        check(o.open(path).empty(), "open the 9 MiB file");
        std::string want, line;
        uint64_t x = 88172645463325252ull;
        for (uint64_t i = 0; want.size() < (9u << 20); i++) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            size_t len = (size_t)(x % 300000);
            const size_t have = o.text().size();  // every seventh line fills the buffer to the threshold - 1, + 0, + 1
            if (i % 7 == 6 && have + 2 <= OutFile::FLUSH_AT) len = OutFile::FLUSH_AT - have - 2 + (size_t)(i / 7 % 3);
            line.assign(len, (char)('a' + i % 26));
            line += '\n';
            if (i % 5 == 3) {
                const std::vector<std::string> pieces = {line.substr(0, line.size() / 2), "", line.substr(line.size() / 2)};
                check(o.write(pieces), "pieces into the 9 MiB file");
            } else if (i % 5 == 4) {
                check(o.write(line), "a string into the 9 MiB file");
            } else {
                o.text() += line;
            }
            want += line;
        }
        check(o.close().empty() && o.close().empty(), "close the 9 MiB file, twice");
        check(slurp(path) == want, "the 9 MiB file read back");
        remove(path.c_str());
    }
    remove(scoped.c_str());
    if (!bad) puts("outfile ok");
    return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) {
        fputs(HELP_MAIN, stderr);
        return 2;
    }
    const std::string cmd = argv[1];
    if (cmd == "-h" || cmd == "--help" || cmd == "help") {
        fputs(HELP_MAIN, stdout);
        return 0;
    }
    if (cmd == "-V" || cmd == "--version") {
        puts("kmertools 0.2.1 (MI355X drop-in)");
        return 0;
    }
    if (cmd == "comp") {
        if (argc < 3) usage_error("'kmertools comp' requires a subcommand but one was not provided\n  [subcommands: oligo, cgr, help]");
        const std::string sub = argv[2];
        if (sub == "oligo") return cmd_oligo(argc, argv, 3);
        if (sub == "cgr") return cmd_cgr(argc, argv, 3);
        usage_error("unrecognized subcommand '" + sub + "'");
    }
    if (cmd == "ctr") return cmd_ctr(argc, argv, 2);
    if (cmd == "debug-read") return cmd_debug_read(argc, argv, 2);
    if (cmd == "debug-fixed6") return cmd_debug_fixed6(argc, argv, 2);
    if (cmd == "debug-outfile") return cmd_debug_outfile(argc, argv, 2);  // debug-outfile <dir>
    if (cmd == "debug-prefilter") return cmd_debug_prefilter(argc, argv, 2);  // debug-prefilter <dir>
    if (cmd == "debug-emit") {  // debug-emit <rows> <bins> <norm 0|1> <threads> <reps>
        if (argc < 7) return 2;
        const double s = debug_emit_bench(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), atoi(argv[4]) != 0,
                                          atoi(argv[5]), atoi(argv[6]));
        printf("best %.3f s\n", s);
        return 0;
    }
    if (cmd == "cov") return cmd_cov(argc, argv, 2);
    if (cmd == "min") return cmd_min(argc, argv, 2);
    if (cmd == "filter") return cmd_filter(argc, argv, 2);
    if (cmd == "correct") return cmd_correct(argc, argv, 2);
    if (cmd == "compare") return cmd_compare(argc, argv, 2);
    if (cmd == "profile") return cmd_profile(argc, argv, 2);
    if (cmd == "sketch") return cmd_sketch(argc, argv, 2);
    if (cmd == "card") return cmd_card(argc, argv, 2);
    if (cmd == "setop") return cmd_setop(argc, argv, 2);
    if (cmd == "graph") return cmd_graph(argc, argv, 2);
    if (cmd == "unitigs") return cmd_unitigs(argc, argv, 2);
    if (cmd == "hetmers") return cmd_hetmers(argc, argv, 2);
    if (cmd == "thread") return cmd_thread(argc, argv, 2);
    usage_error("unrecognized subcommand '" + cmd + "'");
}
