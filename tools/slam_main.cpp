// slam_main.cpp -> k-slam_amd/SLAM: the reference's command line over the C ABI (the OUTER drop-in boundary,
// SURVEY.md section 8b last row).  Plain C++ + getopt_long, no Boost; links libkslam_hip.so and nothing else.
//
// Replaces, in the reference (citations into /root/reference/):
//   main                              src/main.cpp:24-157   flags, defaults, dispatch
//   metagenomicAnalysis_Low_Mem       src/SLAM.h:159-268    open files, batch loop, end-of-run outputs
//   metagenomicAnalysis               src/SLAM.h:82-157     (--num-reads-at-once 4294967295: one batch of --num-reads)
//   createIndexFromFASTA              src/GenbankTools.h:224-260   (--parse-fasta)
//   log                               src/sequenceTools.h:171-179  (./log.txt, "[t = 0.00s]\t<message>")
// Same flag names and defaults (src/main.cpp:36-71), same files: <sam-file>, <output-file>, <output-file>_abbreviated,
// <output-file>_PerRead, ./log.txt.  Not built: --parse-genbank, --parse-taxonomy, --server (database builders and a
// dead code path, out of the hot path's scope).
//
//   SLAM [option] --db=DATABASE R1FILE [R2FILE]
//
// Options that `SLAM --help` does not list yet (its text is pinned by tests/golden/slam_help.txt):
//   --sam-sorted        write --sam-file as a coordinate-sorted BAM (include/kslam_bamsort.h): implies --sam-bam, needs --sam-file;
//                       the records stay on the GPU until the last batch, the file is written behind it
//   --sam-index arg     where its BAI index goes (needs --sam-sorted); default: <sam-file>.bai
//   --indels-out arg    write the insertions and deletions the reads carry, left-normalised, to this file as VCF
//                       (include/kslam_indels.h); implies what --variants-out implies
//   --indels-min-alt arg (=2), --indels-min-depth arg (=1)   its filter (need --indels-out)
//   --gunzip            read R1FILE / R2FILE that are plain gzip (RFC 1952: gzip, pigz, `cat a.gz b.gz`), inflated in parallel on
//                       the GPU (include/kslam_gunzip.h); each file on its own, BGZF keeps its own path.  Without it plain gzip
//                       is refused
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <functional>
#include <getopt.h>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>

#include "../include/kslam_bam.h"
#include "../include/kslam_bgzf.h"
#include "../include/kslam_db.h"
#include "../include/kslam_inflate.h"
#include "../include/kslam_gunzip.h"
#include "../include/kslam_samseq.h"
#include "../include/kslam_samunmapped.h"
#include "../include/kslam_readsplit.h"
#include "../include/kslam_coverage.h"
#include "../include/kslam_kreport.h"
#include "../include/kslam_readqc.h"
#include "../include/kslam_samtext.h"
#include "../include/kslam_taxreads.h"
#include "../include/kslam_variants.h"
#include "../include/kslam_indels.h"
#include "../include/kslam_consensus.h"
#include "../include/kslam_bamsort.h"
#include "../include/kslam_depth.h"
#include "../include/kslam_genes.h"
#include "../include/kslam_alignqc.h"
#include "../include/kslam_stream.h"

namespace {

// src/sequenceTools.h:140-179: a Log that opens ./log.txt on first use, fixed notation, two decimals
struct Log {
  FILE *f = nullptr;
  std::chrono::steady_clock::time_point t0;
  void line(const std::string &s) {
    if (!f) {
      f = fopen("log.txt", "w");
      if (!f) {
        fprintf(stderr, "unable to open log file\n");
        exit(1);
      }
      t0 = std::chrono::steady_clock::now();
    }
    const double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    fprintf(f, "[t = %.2fs]\t%s\n", t, s.c_str());
    fflush(f);
  }
};
Log g_log;
void logl(const std::string &s) { g_log.line(s); }

[[noreturn]] void die(const std::string &m) {
  fprintf(stderr, "SLAM: %s\n", m.c_str());
  logl("error: " + m);
  exit(1);
}

struct Options {
  std::string db, out, sam, classified_out, unclassified_out, coverage_out, variants_out, kraken_report;
  uint32_t variants_min_alt = 2, variants_min_depth = 1;
  std::string indels_out;                  // --indels-out (include/kslam_indels.h)
  uint32_t indels_min_alt = 2, indels_min_depth = 1;
  bool indels_min_alt_given = false, indels_min_depth_given = false;
  bool variants_min_alt_given = false, variants_min_depth_given = false;
  bool sam_sorted = false;                 // --sam-sorted (include/kslam_bamsort.h)
  bool gunzip = false;                     // --gunzip (include/kslam_gunzip.h)
  std::string sam_index;                   // --sam-index
  std::string consensus_out;               // --consensus-out (include/kslam_consensus.h)
  kslam_consensus_params consensus{1, 500, KSLAM_CONSENSUS_FILL_N, 1};
  const char *consensus_dependent = nullptr;   // the first of --consensus-min-depth / -call-permille / -fill / -min-covered given
  std::string depth_out;                   // --depth-out (include/kslam_depth.h)
  std::string genes_out;                   // --genes-out (include/kslam_genes.h)
  uint32_t depth_min = 1;
  bool depth_min_given = false;
  std::string qc_out;                      // --qc-out (include/kslam_readqc.h)
  uint32_t qc_max_cycles = 0;
  bool qc_max_cycles_given = false;
  std::string align_qc_out;                // --align-qc-out (include/kslam_alignqc.h)
  uint32_t align_qc_max_cycles = 0;
  bool align_qc_max_cycles_given = false;
  bool reads_out_bgzf = false;
  std::string extract_out;                 // --extract-out (include/kslam_taxreads.h)
  std::vector<uint32_t> extract_taxids;    // --extract-taxid, repeatable and comma lists
  bool extract_children = false, extract_parents = false, extract_exclude = false;
  uint32_t score_threshold = 0, match = 2, mismatch = 3, gap_open = 5, gap_extend = 2;
  uint32_t num_reads = UINT32_MAX, num_reads_at_once = 10000000, num_alignments = 10;
  double score_fraction = 0.95;
  bool sam_xa = false, just_align = false, no_pseudo = false, help = false, version = false, parse_fasta = false, sam_bgzf = false,
       sam_bam = false, sam_seq = false, sam_unmapped = false, sam_deflate_given = false;
  int sam_deflate = KSLAM_BGZF_DEFLATE_FIXED;
  int device = 0;
  std::vector<std::string> inputs;
};

uint32_t to_u32(const char *s, const char *name) {
  char *end = nullptr;
  errno = 0;
  const unsigned long long v = strtoull(s, &end, 10);
  if (errno || !end || *end || end == s || v > UINT32_MAX || s[0] == '-') die(std::string("the argument ('") + s + "') for option '--" + name + "' is invalid");
  return (uint32_t)v;
}

void usage(FILE *o) {
  // src/main.cpp:102-113 + the option table of :36-71
  fputs("Usage\tSLAM [option] --db=DATABASE R1FILE R2FILE\n"
        "\tAlign paired reads from R1FILE and R2FILE against DATABASE and perform metagenomic analysis\n"
        "or\tSLAM [option] --db=DATABASE R1FILE\n"
        "\tAlign reads from R1FILE against DATABASE and perform metagenomic analysis\n"
        "\tR1FILE and R2FILE are FASTQ text or BGZF (bgzip-style .fastq.gz, inflated on the GPU), each on its own\n"
        "Allowed options:\n"
        "  --help                                produce help message\n"
        "  --db arg                              SLAM database directory which reads will be aligned against\n"
        "  --min-alignment-score arg (=0)        alignment score cutoff\n"
        "  --score-fraction-threshold arg (=0.95) screen alignments with scores < this*top score\n"
        "  --match-score arg (=2)                match score\n"
        "  --mismatch-penalty arg (=3)           mismatch penalty (positive)\n"
        "  --gap-open arg (=5)                   gap opening penalty (positive)\n"
        "  --gap-extend arg (=2)                 gap extend penalty (positive)\n"
        "  --num-reads arg (=4294967295)         Number of reads from R1/R2 File to align\n"
        "  --num-reads-at-once arg (=10000000)   Reduce RAM usage by only analysing \"arg\" reads at once, this will increase execution time\n"
        "  --output-file arg                     write to this file instead of stdout\n"
        "  --sam-file arg                        write SAM output to this file\n"
        "  --num-alignments arg (=10)            Number of alignments to report in SAM file\n"
        "  --sam-xa                              only output primary alignment lines, use XA field for secondary alignments\n"
        "  --version                             print version number\n"
        "  --just-align                          only perform alignments, not metagenomics\n"
        "  --no-pseudo-assembly                  do not link alignments together\n"
        "  --sam-bgzf                            write --sam-file as BGZF (blocked gzip, as bgzip writes it)\n"
        "  --sam-bam                             write --sam-file as BAM (implies --sam-bgzf)\n"
        "  --sam-deflate arg (=fixed)            fixed or dynamic: the Huffman codes of --sam-bgzf / --sam-bam (dynamic: a smaller file)\n"
        "  --sam-seq                             write SEQ and QUAL on the primary rows of --sam-file instead of \"*\"\n"
        "  --sam-unmapped                        after each batch's rows, write a FLAG-4 row to --sam-file for every read without an\n"
        "                                        alignment; with --sam-seq the file is then a full copy of the reads\n"
        "  --classified-out arg                  write the classified reads (with --just-align: the aligned reads) to this FASTQ file;\n"
        "                                        with R1FILE and R2FILE arg must contain a '#', replaced by 1 and 2\n"
        "  --unclassified-out arg                the same for the reads that are not classified\n"
        "  --reads-out-bgzf                      write those files as BGZF (--sam-deflate applies)\n"
        "  --coverage-out arg                    write a per-entry coverage table to this file: alignments, unique read pairs,\n"
        "                                        aligned and covered bases, breadth and mean depth (works with --just-align)\n"
        "  --kraken-report arg                   write a Kraken-style report to this file: percent, clade reads, direct reads, rank code,\n"
        "                                        taxonomy id and indented name per taxon, as Bracken, Pavian, Krona and MultiQC read it\n"
        "  --extract-taxid arg                   choose a taxonomy id (repeatable; a comma list is accepted): the reads classified to it go\n"
        "                                        to --extract-out, as KrakenTools' extract_kraken_reads.py -t writes them\n"
        "  --extract-out arg                     the FASTQ file for the reads of the chosen taxa; with R1FILE and R2FILE arg must contain\n"
        "                                        a '#', replaced by 1 and 2 (--reads-out-bgzf and --sam-deflate apply)\n"
        "  --extract-include-children            also the reads of every taxon below a chosen one\n"
        "  --extract-include-parents             also the reads of every taxon on the way from a chosen one up to the root\n"
        "  --extract-exclude                     write every read that does NOT match instead (reads without alignment included)\n"
        "  --variants-out arg                    write the single-base differences between the reads and the entries to this file as\n"
        "                                        VCF 4.2 (sites only: DP, AO, SAF, SAR, AF); works with --just-align, needs no --sam-file\n"
        "  --variants-min-alt arg (=2)           report a site only when at least arg reads carry the alternate base\n"
        "  --variants-min-depth arg (=1)         report a site only when at least arg reads cover it\n"
        "  --consensus-out arg                   write the consensus sequence of every entry the reads cover to this file as FASTA, called\n"
        "                                        per position from the pile-up with substitutions, deletions and insertions (as samtools\n"
        "                                        consensus gives); works with --just-align and single-end, needs no --sam-file\n"
        "  --consensus-min-depth arg (=1)        call a position only when at least arg reads cover it (at least 1)\n"
        "  --consensus-call-permille arg (=500)  call a base, a deletion or an insertion only when more than arg of 1000 reads at the\n"
        "                                        position carry it (500 to 999); else N\n"
        "  --consensus-fill arg (=n)             n: write N where the depth is below --consensus-min-depth; ref: the entry's own base\n"
        "  --consensus-min-covered arg (=1)      write an entry only when at least arg of its positions are covered\n"
        "  --depth-out arg                       write the depth along every entry to this file as bedGraph (locus, start, end, depth;\n"
        "                                        0-based, half-open, as bedtools genomecov -bg); works with --just-align, needs no --sam-file\n"
        "  --depth-min arg (=1)                  write only the runs whose depth is at least arg\n"
        "  --genes-out arg                       write a per-gene abundance table to this file: alignments, unique read pairs,\n"
        "                                        overlapping bases, RPK and TPM per annotated gene (works with --just-align)\n"
        "  --qc-out arg                          write a QC report on the reads taken in to this file as JSON: reads, bases, lengths, base\n"
        "                                        content and quality per cycle, mean quality per read, GC content, Q20 / Q30 rates;\n"
        "                                        works with --just-align, needs no --sam-file\n"
        "  --qc-max-cycles arg (=512)            per-cycle rows of --qc-out, 1 to 65536; later cycles are pooled in one more row\n"
        "  --align-qc-out arg                    write a QC report on the alignments to this file as JSON: error rate by cycle and by base\n"
        "                                        quality, substitutions, indel lengths, edit distance, identity, insert sizes; works with\n"
        "                                        --just-align and single-end, needs no --sam-file\n"
        "  --align-qc-max-cycles arg (=512)      per-cycle rows of --align-qc-out, 1 to 65536; later cycles are pooled in one more row\n"
        "\n", o);
}

Options parse(int argc, char **argv) {
  Options o;
  enum { DB = 256, MINSCORE, FRACTION, MATCH, MISMATCH, GAPO, GAPE, NREADS, ATONCE, OUT, SAM, NALIGN, XA, VERSION, JUST, NOPSEUDO, HELP, INPUT,
         PARSE_FASTA, UNSUPPORTED, DEVICE, IGNORED, SAM_BGZF, SAM_BAM, SAM_SORTED, SAM_INDEX, GUNZIP, SAM_SEQ, SAM_UNMAPPED, SAM_DEFLATE, CLASSIFIED_OUT, UNCLASSIFIED_OUT, READS_OUT_BGZF, COVERAGE_OUT,
         VARIANTS_OUT, VARIANTS_MIN_ALT, VARIANTS_MIN_DEPTH, INDELS_OUT, INDELS_MIN_ALT, INDELS_MIN_DEPTH, CONSENSUS_OUT, CONSENSUS_MIN_DEPTH, CONSENSUS_PERMILLE, CONSENSUS_FILL, CONSENSUS_MIN_COVERED, DEPTH_OUT, DEPTH_MIN, GENES_OUT, QC_OUT, QC_MAX_CYCLES, ALIGN_QC_OUT, ALIGN_QC_MAX_CYCLES, KRAKEN_REPORT, EXTRACT_TAXID, EXTRACT_OUT, EXTRACT_CHILDREN, EXTRACT_PARENTS, EXTRACT_EXCLUDE };
  static const option longopts[] = {
      {"db", required_argument, nullptr, DB}, {"min-alignment-score", required_argument, nullptr, MINSCORE},
      {"score-fraction-threshold", required_argument, nullptr, FRACTION}, {"match-score", required_argument, nullptr, MATCH},
      {"mismatch-penalty", required_argument, nullptr, MISMATCH}, {"gap-open", required_argument, nullptr, GAPO},
      {"gap-extend", required_argument, nullptr, GAPE}, {"num-reads", required_argument, nullptr, NREADS},
      {"num-reads-at-once", required_argument, nullptr, ATONCE}, {"output-file", required_argument, nullptr, OUT},
      {"sam-file", required_argument, nullptr, SAM}, {"num-alignments", required_argument, nullptr, NALIGN},
      {"sam-xa", no_argument, nullptr, XA}, {"version", no_argument, nullptr, VERSION}, {"just-align", no_argument, nullptr, JUST},
      {"no-pseudo-assembly", no_argument, nullptr, NOPSEUDO}, {"help", no_argument, nullptr, HELP},
      {"input-file", required_argument, nullptr, INPUT}, {"parse-fasta", no_argument, nullptr, PARSE_FASTA},
      {"parse-genbank", no_argument, nullptr, UNSUPPORTED}, {"parse-taxonomy", no_argument, nullptr, UNSUPPORTED},
      {"server", no_argument, nullptr, UNSUPPORTED}, {"alignment-only", no_argument, nullptr, IGNORED},   // declared, never read (src/main.cpp:80-82)
      {"device", required_argument, nullptr, DEVICE},   // not in the reference: the HIP device ordinal (default 0)
      {"sam-bgzf", no_argument, nullptr, SAM_BGZF},     // not in the reference: the SAM file as BGZF (include/kslam_bgzf.h)
      {"sam-bam", no_argument, nullptr, SAM_BAM},       // not in the reference: the SAM file as BAM (include/kslam_bam.h)
      // not in the reference: the SAM file as a coordinate-sorted BAM with its BAI index (include/kslam_bamsort.h)
      {"sam-sorted", no_argument, nullptr, SAM_SORTED}, {"sam-index", required_argument, nullptr, SAM_INDEX},
      {"gunzip", no_argument, nullptr, GUNZIP},   // not in the reference: plain gzip input (include/kslam_gunzip.h)
      {"sam-deflate", required_argument, nullptr, SAM_DEFLATE},   // not in the reference: kslam_set_bgzf_deflate (include/kslam_bgzf.h)
      {"sam-seq", no_argument, nullptr, SAM_SEQ},       // not in the reference: SEQ and QUAL in the SAM file (include/kslam_samseq.h)
      {"sam-unmapped", no_argument, nullptr, SAM_UNMAPPED},   // not in the reference: rows for the reads without alignment (include/kslam_samunmapped.h)
      // not in the reference: the reads themselves, split by outcome (include/kslam_readsplit.h; Kraken 2's option names)
      {"classified-out", required_argument, nullptr, CLASSIFIED_OUT}, {"unclassified-out", required_argument, nullptr, UNCLASSIFIED_OUT},
      {"reads-out-bgzf", no_argument, nullptr, READS_OUT_BGZF},
      {"coverage-out", required_argument, nullptr, COVERAGE_OUT},   // not in the reference: include/kslam_coverage.h
      // not in the reference: include/kslam_variants.h
      {"variants-out", required_argument, nullptr, VARIANTS_OUT}, {"variants-min-alt", required_argument, nullptr, VARIANTS_MIN_ALT},
      {"variants-min-depth", required_argument, nullptr, VARIANTS_MIN_DEPTH},
      // not in the reference: include/kslam_indels.h
      {"indels-out", required_argument, nullptr, INDELS_OUT}, {"indels-min-alt", required_argument, nullptr, INDELS_MIN_ALT},
      {"indels-min-depth", required_argument, nullptr, INDELS_MIN_DEPTH},
      // not in the reference: include/kslam_consensus.h
      {"consensus-out", required_argument, nullptr, CONSENSUS_OUT}, {"consensus-min-depth", required_argument, nullptr, CONSENSUS_MIN_DEPTH},
      {"consensus-call-permille", required_argument, nullptr, CONSENSUS_PERMILLE}, {"consensus-fill", required_argument, nullptr, CONSENSUS_FILL},
      {"consensus-min-covered", required_argument, nullptr, CONSENSUS_MIN_COVERED},
      {"depth-out", required_argument, nullptr, DEPTH_OUT}, {"depth-min", required_argument, nullptr, DEPTH_MIN},   // not in the reference: include/kslam_depth.h
      {"genes-out", required_argument, nullptr, GENES_OUT},   // not in the reference: include/kslam_genes.h
      {"qc-out", required_argument, nullptr, QC_OUT}, {"qc-max-cycles", required_argument, nullptr, QC_MAX_CYCLES},   // not in the reference: include/kslam_readqc.h
      // not in the reference: include/kslam_alignqc.h
      {"align-qc-out", required_argument, nullptr, ALIGN_QC_OUT}, {"align-qc-max-cycles", required_argument, nullptr, ALIGN_QC_MAX_CYCLES},
      {"kraken-report", required_argument, nullptr, KRAKEN_REPORT},   // not in the reference: include/kslam_kreport.h (Kraken 2's --report)
      // not in the reference: include/kslam_taxreads.h (KrakenTools' extract_kraken_reads.py)
      {"extract-taxid", required_argument, nullptr, EXTRACT_TAXID}, {"extract-out", required_argument, nullptr, EXTRACT_OUT},
      {"extract-include-children", no_argument, nullptr, EXTRACT_CHILDREN}, {"extract-include-parents", no_argument, nullptr, EXTRACT_PARENTS},
      {"extract-exclude", no_argument, nullptr, EXTRACT_EXCLUDE},
      {nullptr, 0, nullptr, 0}};
  opterr = 0;
  int c;
  // a leading '-' in the option string: positional arguments arrive in order as option 1 (boost's positional "input-file")
  while ((c = getopt_long(argc, argv, "-", longopts, nullptr)) != -1) {
    switch (c) {
      case 1: o.inputs.push_back(optarg); break;
      case INPUT: o.inputs.push_back(optarg); break;
      case DB: o.db = optarg; break;
      case MINSCORE: o.score_threshold = to_u32(optarg, "min-alignment-score"); break;
      case FRACTION: {
        char *end = nullptr;
        o.score_fraction = strtod(optarg, &end);
        if (!end || *end || end == optarg) die(std::string("the argument ('") + optarg + "') for option '--score-fraction-threshold' is invalid");
        break;
      }
      case MATCH: o.match = to_u32(optarg, "match-score"); break;
      case MISMATCH: o.mismatch = to_u32(optarg, "mismatch-penalty"); break;
      case GAPO: o.gap_open = to_u32(optarg, "gap-open"); break;
      case GAPE: o.gap_extend = to_u32(optarg, "gap-extend"); break;
      case NREADS: o.num_reads = to_u32(optarg, "num-reads"); break;
      case ATONCE: o.num_reads_at_once = to_u32(optarg, "num-reads-at-once"); break;
      case OUT: o.out = optarg; break;
      case SAM: o.sam = optarg; break;
      case NALIGN: o.num_alignments = to_u32(optarg, "num-alignments"); break;
      case XA: o.sam_xa = true; break;
      case SAM_BGZF: o.sam_bgzf = true; break;
      case SAM_BAM: o.sam_bam = true; break;
      case SAM_SORTED: o.sam_sorted = true; break;
      case SAM_INDEX: o.sam_index = optarg; break;
      case GUNZIP: o.gunzip = true; break;
      case SAM_SEQ: o.sam_seq = true; break;
      case SAM_UNMAPPED: o.sam_unmapped = true; break;
      case CLASSIFIED_OUT: o.classified_out = optarg; break;
      case UNCLASSIFIED_OUT: o.unclassified_out = optarg; break;
      case READS_OUT_BGZF: o.reads_out_bgzf = true; break;
      case COVERAGE_OUT: o.coverage_out = optarg; break;
      case VARIANTS_OUT: o.variants_out = optarg; break;
      case INDELS_OUT: o.indels_out = optarg; break;
      case INDELS_MIN_ALT: o.indels_min_alt = to_u32(optarg, "indels-min-alt"); o.indels_min_alt_given = true; break;
      case INDELS_MIN_DEPTH: o.indels_min_depth = to_u32(optarg, "indels-min-depth"); o.indels_min_depth_given = true; break;
      case CONSENSUS_OUT: o.consensus_out = optarg; break;
      case CONSENSUS_MIN_DEPTH:
        o.consensus.min_depth = to_u32(optarg, "consensus-min-depth");
        if (o.consensus.min_depth < 1) die(std::string("the argument ('") + optarg + "') for option '--consensus-min-depth' is invalid: at least 1");
        if (!o.consensus_dependent) o.consensus_dependent = "consensus-min-depth";
        break;
      case CONSENSUS_PERMILLE:
        o.consensus.call_permille = to_u32(optarg, "consensus-call-permille");
        if (o.consensus.call_permille < 500 || o.consensus.call_permille > 999)
          die(std::string("the argument ('") + optarg + "') for option '--consensus-call-permille' is invalid: 500 to 999");
        if (!o.consensus_dependent) o.consensus_dependent = "consensus-call-permille";
        break;
      case CONSENSUS_FILL:
        if (strcmp(optarg, "n") != 0 && strcmp(optarg, "ref") != 0)
          die(std::string("the argument ('") + optarg + "') for option '--consensus-fill' is invalid");
        o.consensus.fill = strcmp(optarg, "ref") == 0 ? KSLAM_CONSENSUS_FILL_REF : KSLAM_CONSENSUS_FILL_N;
        if (!o.consensus_dependent) o.consensus_dependent = "consensus-fill";
        break;
      case CONSENSUS_MIN_COVERED:
        o.consensus.min_covered = to_u32(optarg, "consensus-min-covered");
        if (!o.consensus_dependent) o.consensus_dependent = "consensus-min-covered";
        break;
      case DEPTH_OUT: o.depth_out = optarg; break;
      case GENES_OUT: o.genes_out = optarg; break;
      case DEPTH_MIN: o.depth_min = to_u32(optarg, "depth-min"); o.depth_min_given = true; break;
      case KRAKEN_REPORT: o.kraken_report = optarg; break;
      case ALIGN_QC_OUT: o.align_qc_out = optarg; break;
      case ALIGN_QC_MAX_CYCLES:
        o.align_qc_max_cycles = to_u32(optarg, "align-qc-max-cycles");
        if (o.align_qc_max_cycles < 1 || o.align_qc_max_cycles > KSLAM_ALIGN_QC_MAX_CYCLES)
          die(std::string("the argument ('") + optarg + "') for option '--align-qc-max-cycles' is invalid: 1 to 65536");
        o.align_qc_max_cycles_given = true;
        break;
      case QC_OUT: o.qc_out = optarg; break;
      case QC_MAX_CYCLES:
        o.qc_max_cycles = to_u32(optarg, "qc-max-cycles");
        if (o.qc_max_cycles < 1 || o.qc_max_cycles > KSLAM_READ_QC_MAX_CYCLES)
          die(std::string("the argument ('") + optarg + "') for option '--qc-max-cycles' is invalid: 1 to 65536");
        o.qc_max_cycles_given = true;
        break;
      case EXTRACT_OUT: o.extract_out = optarg; break;
      case EXTRACT_CHILDREN: o.extract_children = true; break;
      case EXTRACT_PARENTS: o.extract_parents = true; break;
      case EXTRACT_EXCLUDE: o.extract_exclude = true; break;
      case EXTRACT_TAXID: {   // one id or a comma list; every piece a number other than 0
        const std::string arg = optarg;
        size_t at = 0;
        for (;;) {
          const size_t comma = arg.find(',', at);
          const std::string piece = arg.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
          const uint32_t id = to_u32(piece.c_str(), "extract-taxid");
          if (id == 0) die("the argument ('" + arg + "') for option '--extract-taxid' is invalid: taxonomy id 0 cannot be chosen (see '--unclassified-out')");
          o.extract_taxids.push_back(id);
          if (comma == std::string::npos) break;
          at = comma + 1;
        }
        break;
      }
      case VARIANTS_MIN_ALT: o.variants_min_alt = to_u32(optarg, "variants-min-alt"); o.variants_min_alt_given = true; break;
      case VARIANTS_MIN_DEPTH: o.variants_min_depth = to_u32(optarg, "variants-min-depth"); o.variants_min_depth_given = true; break;
      case SAM_DEFLATE:
        if (strcmp(optarg, "fixed") != 0 && strcmp(optarg, "dynamic") != 0)
          die(std::string("the argument ('") + optarg + "') for option '--sam-deflate' is invalid");
        o.sam_deflate = strcmp(optarg, "dynamic") == 0 ? KSLAM_BGZF_DEFLATE_DYNAMIC : KSLAM_BGZF_DEFLATE_FIXED;
        o.sam_deflate_given = true;
        break;
      case VERSION: o.version = true; break;
      case JUST: o.just_align = true; break;
      case NOPSEUDO: o.no_pseudo = true; break;
      case HELP: o.help = true; break;
      case PARSE_FASTA: o.parse_fasta = true; break;
      case DEVICE: o.device = (int)to_u32(optarg, "device"); break;
      case IGNORED: break;
      case UNSUPPORTED: die("the database builders --parse-genbank / --parse-taxonomy and --server are not part of this build");
      default: die(std::string("unrecognised option '") + (optind > 0 && optind <= argc ? argv[optind - 1] : "?") + "'");
    }
  }
  if (o.sam_deflate_given && !o.sam_bgzf && !o.sam_bam && !o.sam_sorted && !o.reads_out_bgzf) die("option '--sam-deflate' needs '--sam-bgzf' or '--sam-bam'");
  if (o.sam_unmapped && o.sam.empty()) die("option '--sam-unmapped' needs '--sam-file'");
  if (o.sam_sorted && o.sam.empty()) die("option '--sam-sorted' needs '--sam-file'");
  if (!o.sam_index.empty() && !o.sam_sorted) die("option '--sam-index' needs '--sam-sorted'");
  if (o.sam_sorted) o.sam_bam = true;                                   // --sam-sorted implies --sam-bam
  if (o.sam_sorted && o.sam_index.empty()) o.sam_index = o.sam + ".bai";
  if (!o.kraken_report.empty() && o.just_align) die("option '--kraken-report' cannot be combined with '--just-align': the report counts taxonomy ids");
  if (o.just_align && (!o.extract_taxids.empty() || !o.extract_out.empty()))
    die(std::string("option '--") + (o.extract_taxids.empty() ? "extract-out" : "extract-taxid") + "' cannot be combined with '--just-align': the reads are chosen by taxonomy id");
  if (!o.extract_taxids.empty() && o.extract_out.empty()) die("option '--extract-taxid' needs '--extract-out'");
  if (o.extract_taxids.empty() && !o.extract_out.empty()) die("option '--extract-out' needs '--extract-taxid'");
  if (o.extract_children && o.extract_taxids.empty()) die("option '--extract-include-children' needs '--extract-taxid'");
  if (o.extract_parents && o.extract_taxids.empty()) die("option '--extract-include-parents' needs '--extract-taxid'");
  if (o.extract_exclude && o.extract_taxids.empty()) die("option '--extract-exclude' needs '--extract-taxid'");
  if (o.variants_min_alt_given && o.variants_out.empty()) die("option '--variants-min-alt' needs '--variants-out'");
  if (o.variants_min_depth_given && o.variants_out.empty()) die("option '--variants-min-depth' needs '--variants-out'");
  if (o.indels_min_alt_given && o.indels_out.empty()) die("option '--indels-min-alt' needs '--indels-out'");
  if (o.indels_min_depth_given && o.indels_out.empty()) die("option '--indels-min-depth' needs '--indels-out'");
  if (o.consensus_dependent && o.consensus_out.empty()) die(std::string("option '--") + o.consensus_dependent + "' needs '--consensus-out'");
  if (o.depth_min_given && o.depth_out.empty()) die("option '--depth-min' needs '--depth-out'");
  if (o.qc_max_cycles_given && o.qc_out.empty()) die("option '--qc-max-cycles' needs '--qc-out'");
  if (o.align_qc_max_cycles_given && o.align_qc_out.empty()) die("option '--align-qc-max-cycles' needs '--align-qc-out'");
  return o;
}

struct FileText {   // a whole file in memory -- page-locked (DMA straight from it) unless `pageable`; empty when missing
  char *p = nullptr;
  uint64_t len = 0, cap = 0;
  bool good = false, pageable = false;
  explicit FileText(bool pageable_ = false) : pageable(pageable_) {}
  char *get(uint64_t bytes) { return (char *)(pageable ? malloc(bytes) : kslam_host_alloc(bytes)); }
  void load(const std::string &path) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return;
    struct stat sb;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {   // a pipe or device: read until EOF into a growing buffer
      std::vector<char> v;
      char buf[1 << 16];
      ssize_t r;
      while ((r = read(fd, buf, sizeof buf)) > 0) v.insert(v.end(), buf, buf + r);
      close(fd);
      cap = v.size() + 64;
      p = get(cap);
      if (!p) die("out of page-locked memory for " + path);
      memcpy(p, v.data(), v.size());
      len = v.size();
      good = true;
      return;
    }
    len = (uint64_t)sb.st_size;
    cap = len + 64;
    p = get(cap);
    if (!p) die("out of page-locked memory for " + path);
    const unsigned n_thr = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(8, len >> 26));
    std::vector<std::thread> th;
    bool ok = true;
    for (unsigned t = 0; t < n_thr; t++)
      th.emplace_back([&, t] {
        uint64_t at = len * t / n_thr;
        const uint64_t end = len * (t + 1) / n_thr;
        while (at < end) {
          const ssize_t r = pread(fd, p + at, (size_t)std::min<uint64_t>(end - at, 1u << 30), (off_t)at);
          if (r <= 0) {
            if (r < 0 && errno == EINTR) continue;
            ok = false;
            return;
          }
          at += (uint64_t)r;
        }
      });
    for (auto &x : th) x.join();
    close(fd);
    if (!ok) die("reading " + path + " failed");
    good = true;
  }
  void release() {
    if (p && owner) kslam_free_pinned(owner, p);
    else if (p && pageable) free(p);
    else if (p) kslam_host_free(p, cap);
    p = nullptr;
    owner = nullptr;
  }
  // A file that starts with the gzip magic is BGZF: its members are inflated on the GPU (include/kslam_inflate.h), the
  // compressed bytes are released, and the run goes on with the text.  Plain gzip ends the run with the scan's message --
  // unless --gunzip was given: then it is inflated on the GPU too, from guessed and proven block starts (include/kslam_gunzip.h).
  kslam_ctx *owner = nullptr;   // set: p is the context's page-locked text (kslam_free_pinned)
  void inflate_if_gzip(kslam_ctx *ctx, const std::string &path, bool gunzip) {
    if (!good || !kslam_bgzf_is_gzip(p, len)) return;
    uint64_t n_members = 0, text_len = 0;
    char *text = nullptr;
    const kslam_status scanned = kslam_bgzf_scan(p, len, &n_members, &text_len);
    if (scanned == KSLAM_ERR_UNSUPPORTED && gunzip) {
      if (kslam_gunzip_inflate(ctx, p, len, &text, &text_len) != KSLAM_OK) die(path + ": " + kslam_last_error(ctx));
    } else {
      if (scanned != KSLAM_OK)
        die(path + ": " + kslam_tail_last_error() + (scanned == KSLAM_ERR_UNSUPPORTED ? "; or read it as it is with --gunzip" : ""));
      if (kslam_bgzf_inflate(ctx, p, len, &text, &text_len) != KSLAM_OK) die(path + ": " + kslam_last_error(ctx));
    }
    release();
    p = text;
    len = text_len;
    owner = ctx;
  }
  ~FileText() { release(); }
};

bool write_file(const std::string &path, const char *p, uint64_t n) {
  const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) return false;
  int user = fd;
  const bool ok = n == 0 || kslam_write_fd(&user, p, n) == 0;
  close(fd);
  return ok;
}

// createIndexFromFASTA, src/GenbankTools.h:224-260: locusTag = the text between '>' and the first space (empty when the
// header has no space, or the space comes first), bases upper-cased, entries without bases dropped, line ends \n, \r\n, \r
int parse_fasta(const Options &o) {
  logl("Parsing FASTA");
  std::vector<std::string> bases, tags;
  for (const std::string &name : o.inputs) {
    logl("Parsing\t" + name);
    FileText t(true);   // no GPU needed for the database builder
    t.load(name);
    if (!t.good) die("unable to open FASTA file");
    std::string cur_b, cur_t;
    auto flush = [&] {
      if (!cur_b.empty()) {
        bases.push_back(std::move(cur_b));
        tags.push_back(cur_t);
      }
      cur_b.clear();
      cur_t.clear();
    };
    uint64_t i = 0;
    while (i < t.len) {   // safeGetline, src/sequenceTools.h:45-73
      uint64_t j = i;
      while (j < t.len && t.p[j] != '\n' && t.p[j] != '\r') j++;
      const char *line = t.p + i;
      const uint64_t n = j - i;
      if (j < t.len && t.p[j] == '\r' && j + 1 < t.len && t.p[j + 1] == '\n') j++;
      i = j + 1;
      if (n == 0) continue;
      if (line[0] == '>') {
        flush();
        const char *sp = (const char *)memchr(line, ' ', n);
        if (sp && sp != line) cur_t.assign(line + 1, sp - line - 1);
      } else {
        cur_b.append(line, n);
      }
    }
    flush();
  }
  for (auto &b : bases)
    for (auto &ch : b) ch = (char)toupper((unsigned char)ch);   // inPlaceConvertToUpperCase, src/sequenceTools.h:117-122
  const uint64_t n = bases.size();
  std::string all_b, all_t;
  std::vector<uint64_t> b_off(n + 1, 0), t_off(n + 1, 0), gene_first(n + 1, 0);
  std::vector<uint32_t> tax(n, 0);
  for (uint64_t e = 0; e < n; e++) {
    all_b += bases[e];
    all_t += tags[e];
    b_off[e + 1] = all_b.size();
    t_off[e + 1] = all_t.size();
  }
  kslam_db_columns c;
  memset(&c, 0, sizeof c);
  c.index.n_entries = n;
  c.index.bases = all_b.data();
  c.index.bases_off = b_off.data();
  c.index.locus_tag = all_t.data();
  c.index.locus_tag_off = t_off.data();
  c.index.taxonomy_id = tax.data();
  c.index.gene_first = gene_first.data();
  if (kslam_db_write(o.out.c_str(), &c, 17) != KSLAM_OK) die(kslam_tail_last_error());
  return 0;
}

std::string cat(const std::string &a, uint64_t v, const std::string &b) { return a + std::to_string(v) + b; }

int run(const Options &o, const std::string &command_line) {
  const std::string r1 = o.inputs[0], r2 = o.inputs.size() > 1 ? o.inputs[1] : std::string();
  const bool paired = !r2.empty(), want_sam = !o.sam.empty();
  // --classified-out / --unclassified-out: with two input files the name carries a '#' that becomes 1 and 2 (Kraken 2's rule)
  std::string reads_out_names[4];
  const bool want_reads_out = !o.classified_out.empty() || !o.unclassified_out.empty();
  for (int k = 0; k < 2; k++) {
    const std::string &name = k ? o.unclassified_out : o.classified_out;
    if (name.empty()) continue;
    const size_t at = name.find('#');
    if (paired && at == std::string::npos) {
      fprintf(stderr, "SLAM: with R1FILE and R2FILE the argument of '--%s' must contain a '#' (replaced by 1 and 2)\n", k ? "unclassified-out" : "classified-out");
      usage(stderr);
      exit(1);
    }
    reads_out_names[2 * k] = paired ? name.substr(0, at) + "1" + name.substr(at + 1) : name;
    if (paired) reads_out_names[2 * k + 1] = name.substr(0, at) + "2" + name.substr(at + 1);
  }
  // --extract-out: the same rule
  std::string extract_names[2];
  const bool want_extract = !o.extract_out.empty();
  if (want_extract) {
    const size_t at = o.extract_out.find('#');
    if (paired && at == std::string::npos) {
      fprintf(stderr, "SLAM: with R1FILE and R2FILE the argument of '--%s' must contain a '#' (replaced by 1 and 2)\n", "extract-out");
      usage(stderr);
      exit(1);
    }
    extract_names[0] = paired ? o.extract_out.substr(0, at) + "1" + o.extract_out.substr(at + 1) : o.extract_out;
    if (paired) extract_names[1] = o.extract_out.substr(0, at) + "2" + o.extract_out.substr(at + 1);
  }
  logl("Performing metagenomic analysis");
  if (o.db.empty()) die("the option '--db' is required but missing");
  // ---- taxDB + database (src/SLAM.h:172-176) ----
  kslam_taxdb *taxdb = nullptr;
  if (!o.just_align) {
    logl("Building taxonomy index");
    FileText t(true);
    t.load(o.db + "/taxDB");
    if (!t.good) die("unable to open taxonomy index file");
    if (kslam_taxdb_parse(t.p, t.len, &taxdb) != KSLAM_OK) die(kslam_tail_last_error());
    logl(cat("Built a taxonomy tree with ", kslam_taxdb_size(taxdb), " nodes"));
  }
  kslam_db *db = nullptr;
  if (kslam_db_load((o.db + "/database").c_str(), 0, &db) != KSLAM_OK) die(std::string("database: ") + kslam_tail_last_error());
  const kslam_db_columns *cols = kslam_db_view(db);
  const kslam_index_view *index = &cols->index;
  kslam_params kp;
  memset(&kp, 0, sizeof kp);
  kp.match = o.match;
  kp.mismatch = o.mismatch;
  kp.gap_open = o.gap_open;
  kp.gap_extend = o.gap_extend;
  kp.score_threshold = o.score_threshold;
  // reportCigar = a SAM file was asked for (src/SLAM.h:169); the variants walk the CIGARs too (the SAM text follows sp.tail.report_cigar)
  kp.report_cigar = (want_sam || !o.variants_out.empty() || !o.indels_out.empty() || !o.consensus_out.empty() || !o.depth_out.empty() || !o.align_qc_out.empty()) ? 1 : 0;
  kp.device = o.device;
  kslam_ctx *ctx = nullptr;
  if (kslam_create(&kp, &ctx) != KSLAM_OK) die(std::string("GPU context: ") + (ctx ? kslam_last_error(ctx) : "kslam_create failed"));
  if (o.sam_bgzf && want_sam && kslam_set_sam_bgzf(ctx, 1) != KSLAM_OK) die(std::string("BGZF: ") + kslam_last_error(ctx));
  if (o.sam_bam && want_sam && kslam_set_sam_bam(ctx, 1) != KSLAM_OK) die(std::string("BAM: ") + kslam_last_error(ctx));
  if (o.reads_out_bgzf && (want_reads_out || want_extract) && kslam_set_reads_out_bgzf(ctx, 1) != KSLAM_OK) die(std::string("reads out: ") + kslam_last_error(ctx));
  if ((want_sam || ((want_reads_out || want_extract) && o.reads_out_bgzf)) && kslam_set_bgzf_deflate(ctx, o.sam_deflate) != KSLAM_OK) die(std::string("BGZF: ") + kslam_last_error(ctx));
  if (o.sam_seq && want_sam && kslam_set_sam_seq(ctx, 1) != KSLAM_OK) die(std::string("SEQ: ") + kslam_last_error(ctx));
  if (o.sam_unmapped && kslam_set_sam_unmapped(ctx, 1) != KSLAM_OK) die(std::string("unmapped rows: ") + kslam_last_error(ctx));
  logl("Getting k-mers from index");
  if (kslam_set_index(ctx, index->n_entries, kslam_db_entry_bases(db), kslam_db_entry_lengths(db)) != KSLAM_OK)
    die(std::string("index: ") + kslam_last_error(ctx));
  // ---- the input streams (src/SLAM.h:178-188): a file that cannot be read is logged and behaves as an empty stream ----
  FileText t1, t2;
  t1.load(r1);
  if (!t1.good) logl("FASTQ file " + r1 + " bad");
  if (paired) {
    t2.load(r2);
    if (!t2.good) logl("FASTQ file " + r2 + " bad");
  }
  t1.inflate_if_gzip(ctx, r1, o.gunzip);
  t2.inflate_if_gzip(ctx, r2, o.gunzip);
  // ---- outputs ----
  int sam_fd = -1, per_read_fd = -1;
  char *header = nullptr;
  uint64_t header_len = 0;
  if (want_sam) {
    sam_fd = open(o.sam.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);   // O_RDWR: the writer may map the file (KSLAM_WRITER=mmap)
    if (sam_fd < 0) die("unable to open SAM file " + o.sam);
    if (kslam_sam_header(index, command_line.c_str(), &header, &header_len) != KSLAM_OK) die(kslam_tail_last_error());
  }
  kslam_taxreport *report = nullptr;
  if (!o.just_align) {
    per_read_fd = open((o.out + "_PerRead").c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (per_read_fd < 0) die("unable to open " + o.out + "_PerRead");
    if (kslam_taxreport_create(&report) != KSLAM_OK) die(kslam_tail_last_error());
  }
  int reads_out_fds[4] = {-1, -1, -1, -1};
  for (int k = 0; k < 4; k++) {
    if (reads_out_names[k].empty()) continue;
    reads_out_fds[k] = open(reads_out_names[k].c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (reads_out_fds[k] < 0) die("unable to open " + reads_out_names[k]);
  }
  if (want_reads_out && kslam_stream_set_reads_out(ctx, reads_out_fds) != KSLAM_OK) die(std::string("reads out: ") + kslam_last_error(ctx));
  // --extract-out: the taxa are chosen on the tree the context holds, so the annotations (they bring the tree) and the pairing
  // are set here, ahead of the loop, which sets both again for itself and the chosen ids behind them
  int extract_fds[2] = {-1, -1};
  if (want_extract) {
    const uint32_t stages = KSLAM_TAIL_INSERT_SCREEN | KSLAM_TAIL_SCORE_SCREEN | (o.no_pseudo ? 0u : (uint32_t)KSLAM_TAIL_PSEUDO_ASM);
    const uint32_t mode = (o.extract_children ? KSLAM_TAXREADS_CHILDREN : 0u) | (o.extract_parents ? KSLAM_TAXREADS_PARENTS : 0u) |
                          (o.extract_exclude ? KSLAM_TAXREADS_EXCLUDE : 0u);
    if (kslam_set_sam_annotations(ctx, index, taxdb) != KSLAM_OK || kslam_set_pairing(ctx, paired ? 1 : 0, o.score_threshold, o.score_fraction, stages) != KSLAM_OK ||
        kslam_set_taxon_reads(ctx, o.extract_taxids.data(), o.extract_taxids.size(), mode) != KSLAM_OK)
      die(std::string("extract: ") + kslam_last_error(ctx));
    for (int k = 0; k < 2; k++) {
      if (extract_names[k].empty()) continue;
      extract_fds[k] = open(extract_names[k].c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
      if (extract_fds[k] < 0) die("unable to open " + extract_names[k]);
    }
    if (kslam_stream_set_taxon_reads(ctx, extract_fds) != KSLAM_OK) die(std::string("extract: ") + kslam_last_error(ctx));
  }
  // the file reports, in the order they are opened and set: the path, "<what>: " of a refusal, "closing <noun> failed", the setter
  struct OutputFile {
    const std::string &path;
    const char *what, *noun;
    std::function<kslam_status(int)> set;
    int fd = -1;
  } output_files[] = {
      {o.coverage_out, "coverage", "the coverage file", [ctx, &o](int fd) { return kslam_stream_set_coverage(ctx, fd); }},
      {o.kraken_report, "Kraken-style report", "the Kraken-style report", [ctx, &o](int fd) { return kslam_stream_set_kreport(ctx, fd); }},
      {o.consensus_out, "consensus", "the consensus file", [ctx, &o](int fd) { return kslam_stream_set_consensus(ctx, fd, &o.consensus); }},
      {o.variants_out, "variants", "the variants file", [ctx, &o](int fd) { return kslam_stream_set_variants(ctx, fd, o.variants_min_alt, o.variants_min_depth); }},
      {o.indels_out, "indels", "the indels file", [ctx, &o](int fd) { return kslam_stream_set_indels(ctx, fd, o.indels_min_alt, o.indels_min_depth); }},
      {o.depth_out, "depth", "the depth file", [ctx, &o](int fd) { return kslam_stream_set_depth(ctx, fd, o.depth_min); }},
      {o.genes_out, "genes", "the gene table", [ctx, &o](int fd) { return kslam_stream_set_genes(ctx, fd); }},
      {o.qc_out, "read QC", "the read QC report", [ctx, &o](int fd) { return kslam_stream_set_read_qc(ctx, fd, o.qc_max_cycles); }},
      {o.align_qc_out, "alignment QC", "the alignment QC report", [ctx, &o](int fd) { return kslam_stream_set_align_qc(ctx, fd, o.align_qc_max_cycles); }},
  };
  for (OutputFile &f : output_files) {
    if (f.path.empty()) continue;
    f.fd = open(f.path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (f.fd < 0) die("unable to open " + f.path);
    if (f.set(f.fd) != KSLAM_OK) die(std::string(f.what) + ": " + kslam_last_error(ctx));
  }
  int sam_index_fd = -1;
  if (o.sam_sorted) {
    sam_index_fd = open(o.sam_index.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (sam_index_fd < 0) die("unable to open " + o.sam_index);
    if (kslam_stream_set_bam_sort(ctx, 1, sam_index_fd) != KSLAM_OK) die(std::string("sorted BAM: ") + kslam_last_error(ctx));
  }
  kslam_stream_params sp;
  memset(&sp, 0, sizeof sp);
  sp.pairs_per_batch = o.num_reads_at_once;
  sp.max_pairs_total = o.num_reads == UINT32_MAX ? 0 : o.num_reads;
  if (o.num_reads_at_once == UINT32_MAX && sp.max_pairs_total) sp.pairs_per_batch = sp.max_pairs_total;   // metagenomicAnalysis: one batch
  sp.tail.score_threshold = o.score_threshold;
  sp.tail.num_sam_alignments = o.num_alignments;
  sp.tail.score_fraction = o.score_fraction;
  sp.tail.pseudo_assembly = o.no_pseudo ? 0 : 1;
  sp.tail.sam_xa = o.sam_xa ? 1 : 0;
  sp.tail.report_cigar = want_sam ? 1 : 0;
  sp.tail.paired = paired ? 1 : 0;
  sp.sam_fd = sam_fd;
  sp.per_read_fd = per_read_fd;
  sp.sam_header = header;
  sp.sam_header_len = header_len;
  if (paired)
    logl("Getting reads from FASTQ files " + r1 + " and " + r2);
  else
    logl("Getting reads from FASTQ file " + r1);
  logl("Aligning reads to database using k = 32");
  uint32_t *tax_ids = nullptr;
  uint64_t n_tax = 0;
  kslam_stream_stats st;
  memset(&st, 0, sizeof st);
  uint64_t n_pairs = 0;
  if (o.num_reads != 0 && sp.pairs_per_batch != 0) {
    const kslam_status rc = kslam_stream_classify(ctx, index, taxdb, report, t1.p ? t1.p : "", t1.len, paired ? (t2.p ? t2.p : "") : nullptr,
                                                  paired ? t2.len : 0, &sp, &tax_ids, &n_tax, &st);
    if (rc != KSLAM_OK) {
      const char *m = kslam_tail_last_error();
      die(std::string("batch loop: ") + (m && *m ? m : kslam_last_error(ctx)));
    }
    n_pairs = st.n_pairs;
  }
  uint64_t sam_file_bytes = st.sam_bytes + header_len;
  struct stat sam_stat;
  if (sam_fd >= 0 && (o.sam_bgzf || o.sam_bam) && fstat(sam_fd, &sam_stat) == 0) sam_file_bytes = (uint64_t)sam_stat.st_size;   // compressed
  if (sam_fd >= 0) close(sam_fd);
  if (sam_index_fd >= 0 && close(sam_index_fd) != 0) die("closing the BAM index failed");
  if (per_read_fd >= 0) close(per_read_fd);
  for (int fd : reads_out_fds)
    if (fd >= 0 && close(fd) != 0) die("closing a reads-out file failed");
  for (int fd : extract_fds)
    if (fd >= 0 && close(fd) != 0) die("closing a file of extracted reads failed");
  for (const OutputFile &f : output_files)
    if (f.fd >= 0 && close(f.fd) != 0) die(std::string("closing ") + f.noun + " failed");
  logl(cat("Found ", st.n_overlaps, " k-mer overlaps"));
  logl(cat("", st.n_read_pairs_aligned, " entries have k-mer overlaps"));
  if (paired && st.n_batches) logl(cat("Screening all alignment pairs with insert size >= ", st.first_max_insert_size, ""));
  if (want_sam) logl(cat("Writing SAM output (", sam_file_bytes, " bytes)"));
  logl("Processed\t" + std::to_string(n_pairs) + "\t reads");
  if (o.just_align) {
    logl("Done");
  } else {
    // ---- end of run (src/SLAM.h:256-266): <out>_PerRead is complete; <out> and <out>_abbreviated, or the XML on stdout ----
    logl("Combining taxonomies");
    kslam_gene_extras ex = {cols->gene_locus_tag, cols->gene_locus_tag_off, cols->gene_reference, cols->gene_reference_off, cols->gene_id};
    char *xml = nullptr, *abbr = nullptr;
    uint64_t xml_len = 0, abbr_len = 0;
    if (kslam_taxreport_xml(report, index, &ex, taxdb, n_pairs, &xml, &xml_len) != KSLAM_OK) die(kslam_tail_last_error());
    if (!o.out.empty()) {
      if (!write_file(o.out, xml, xml_len)) die("unable to write " + o.out);
      if (kslam_taxonomy_summary(taxdb, tax_ids, n_tax, n_pairs, &abbr, &abbr_len) != KSLAM_OK) die(kslam_tail_last_error());
      if (!write_file(o.out + "_abbreviated", abbr, abbr_len)) die("unable to write " + o.out + "_abbreviated");
    } else {
      fwrite(xml, 1, xml_len, stdout);
    }
    kslam_free(xml);
    kslam_free(abbr);
    logl("Done");
  }
  kslam_free(tax_ids);
  kslam_free(header);
  if (report) kslam_taxreport_free(report);
  t1.release();   // inflated text belongs to the context
  t2.release();
  kslam_destroy(ctx);
  kslam_db_free(db);
  if (taxdb) kslam_taxdb_free(taxdb);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  std::string command_line;   // src/main.cpp:25-30: the @PG line's CL field
  for (int i = 0; i < argc; i++) {
    if (i) command_line += ' ';
    command_line += argv[i];
  }
  const Options o = parse(argc, argv);
  if (o.version) {   // src/main.cpp:95-98
    puts("1.0");
    return 1;
  }
  if (o.help || argc == 1) {
    usage(stdout);
    return 1;
  }
  if (o.parse_fasta) return parse_fasta(o);
  if (o.inputs.size() == 1 || o.inputs.size() == 2) return run(o, command_line);
  return 0;   // src/main.cpp:136: nothing to do without an input file
}
