#!/bin/bash
# CPU-only sanitizer pass over the host stages (database load, FASTQ ingest, host tail, coverage table, unaligned rows, Kraken-style report, reads of chosen taxa, read QC report, per-gene table, alignment QC report, the sorted BAM's record stream and BAI index): the GPU boxes cannot run
# sanitizers, these parts need no GPU.  Builds the two host benches with ASan+UBSan and with TSan and
# runs them on small inputs; any report fails the script.   usage: bash tools/sanitize_host.sh
set -e
cd "$(dirname "$0")/.."
T=$(mktemp -d)
FLAGS="-O1 -g -std=c++17 -pthread -fno-omit-frame-pointer"
g++ $FLAGS -fsanitize=address,undefined tools/tail_bench.cpp k-slam_amd/host/tail.cpp k-slam_amd/host/taxonomy.cpp -o $T/tail_asan
g++ $FLAGS -fsanitize=thread tools/tail_bench.cpp k-slam_amd/host/tail.cpp k-slam_amd/host/taxonomy.cpp -o $T/tail_tsan
g++ $FLAGS -fsanitize=address,undefined tools/fastq_bench.cpp k-slam_amd/host/fastq.cpp -o $T/fq_asan
g++ $FLAGS -fsanitize=thread tools/fastq_bench.cpp k-slam_amd/host/fastq.cpp -o $T/fq_tsan
g++ $FLAGS -fsanitize=address,undefined tools/db_check.cpp k-slam_amd/host/db.cpp k-slam_amd/host/tail.cpp -o $T/db_asan
g++ $FLAGS -fsanitize=thread tools/db_check.cpp k-slam_amd/host/db.cpp k-slam_amd/host/tail.cpp -o $T/db_tsan
g++ $FLAGS -fsanitize=address,undefined tools/coverage_check.cpp k-slam_amd/host/coverage.cpp -o $T/cov_asan
g++ $FLAGS -fsanitize=thread tools/coverage_check.cpp k-slam_amd/host/coverage.cpp -o $T/cov_tsan
g++ $FLAGS -fsanitize=address,undefined tools/samunmapped_check.cpp k-slam_amd/host/samunmapped.cpp k-slam_amd/host/tail.cpp -o $T/su_asan
g++ $FLAGS -fsanitize=address,undefined tools/kreport_check.cpp k-slam_amd/host/kreport.cpp k-slam_amd/host/taxonomy.cpp k-slam_amd/host/tail.cpp -o $T/kr_asan
g++ $FLAGS -fsanitize=address,undefined tools/taxreads_check.cpp k-slam_amd/host/taxreads.cpp k-slam_amd/host/readsplit.cpp k-slam_amd/host/taxonomy.cpp k-slam_amd/host/tail.cpp -o $T/tr_asan
g++ $FLAGS -fsanitize=address,undefined tools/readqc_check.cpp k-slam_amd/host/readqc.cpp k-slam_amd/host/tail.cpp -o $T/rq_asan
g++ $FLAGS -fsanitize=address,undefined tools/genes_check.cpp k-slam_amd/host/genes.cpp -o $T/gn_asan
g++ $FLAGS -fsanitize=address,undefined tools/alignqc_check.cpp k-slam_amd/host/alignqc.cpp -o $T/aq_asan
g++ $FLAGS -fsanitize=address,undefined tools/bamsort_check.cpp k-slam_amd/host/bamsort.cpp -o $T/bs_asan
g++ $FLAGS -fsanitize=address,undefined tools/indels_check.cpp k-slam_amd/host/indels.cpp -o $T/id_asan
export ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1 TSAN_OPTIONS=halt_on_error=1
for mode in 0 1 2; do $T/tail_asan 40000 6 2 $mode > /dev/null; $T/tail_tsan 20000 6 2 $mode > /dev/null; done   # mode 2: the batch loop's two-thread host stage
$T/fq_asan 40000 5 2 > /dev/null
$T/fq_tsan 40000 5 2 > /dev/null
$T/db_asan 150 $T > /dev/null
$T/db_tsan 150 $T > /dev/null
$T/cov_asan 20000 $T > /dev/null
$T/cov_tsan 20000 $T > /dev/null
$T/su_asan 20000 > /dev/null
$T/kr_asan 20000 $T > /dev/null
$T/tr_asan 3000 > /dev/null
$T/rq_asan 4000 $T > /dev/null
$T/gn_asan 20000 $T > /dev/null
$T/aq_asan 20000 $T > /dev/null
$T/bs_asan 20000 > /dev/null
$T/id_asan $T > /dev/null
rm -rf $T
echo "sanitizers: clean (ASan+UBSan, TSan) on the host tail, the FASTQ ingest, the database load, the coverage table, the rows for unaligned reads, the Kraken-style report, the reads of chosen taxa, the read QC report, the per-gene table, the alignment QC report, the sorted BAM's twins and the indel table"
