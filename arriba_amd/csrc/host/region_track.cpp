// arriba_amd/csrc/host/region_track.cpp -- the region track of --rna-metrics (include/arriba_gpu.h: agpu_region_track): the reader of the rRNA interval file
// (--rrna-intervals, BED) and the sweep that turns the genes and exons of a session and those intervals into runs of bases with equal bits (rRNA, coding, exonic, inside a forward /
// a reverse gene) and equal body gene, per contig.  Built once per session and interval file; the host steps rnametrics_core.hpp against it and the device gets a copy.
// It is not the exon index: that index's buckets do not break at CDS boundaries or at gene ends, and they hold members, not classes.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>
#include "arriba_host.h"
#include "../device/rnametrics_core.hpp"

namespace arriba {

agpu_region_track RegionTrack::view() const {
	agpu_region_track v;
	v.id = id;
	v.n_contigs = contig_offset.empty() ? 0 : (uint32_t) (contig_offset.size() - 1); v.contig_offset = contig_offset.data();
	v.n_runs = (uint32_t) run_start.size(); v.run_start = run_start.data(); v.run_bits = run_bits.data(); v.run_gene = run_gene.data(); v.run_rank = run_rank.data();
	v.n_genes = (uint32_t) gene_body.size(); v.gene_body = gene_body.data();
	return v;
}

// BED: contig, start, end (0-based, half open) separated by tabs; further fields are ignored; lines that start with '#', "track" or "browser" and empty lines are skipped
void rrna_intervals_parse(const std::string& path, std::vector<RrnaInterval>& intervals) {
	intervals.clear();
	std::string text;
	{ FILE* file = fopen(path.c_str(), "rb");
	  if (file == nullptr) throw std::runtime_error("--rrna-intervals: cannot read '" + path + "'");
	  char piece[1 << 16];
	  for (size_t got; (got = fread(piece, 1, sizeof(piece), file)) > 0; ) text.append(piece, got);
	  const bool failed = ferror(file) != 0; // (a directory opens and then fails to read)
	  fclose(file);
	  if (failed) throw std::runtime_error("--rrna-intervals: cannot read '" + path + "'"); }
	uint64_t number = 0;
	for (size_t at = 0; at < text.size(); ) {
		size_t end = text.find('\n', at);
		if (end == std::string::npos) end = text.size();
		++number;
		const size_t begin = at;
		at = end + 1;
		if (end > begin && text[end - 1] == '\r') --end;
		if (end == begin || text[begin] == '#' || text.compare(begin, 5, "track") == 0 || text.compare(begin, 7, "browser") == 0) continue;
		const std::string where = "--rrna-intervals: '" + path + "' line " + std::to_string(number) + ": ";
		size_t field_begin[3], field_end[3], from = begin;
		for (int f = 0; f < 3; ++f) {
			if (from > end) throw std::runtime_error(where + "fewer than three fields (contig, start and end, separated by tabs)");
			size_t stop = text.find('\t', from);
			if (stop == std::string::npos || stop > end) stop = end;
			field_begin[f] = from; field_end[f] = stop;
			from = stop + 1;
		}
		if (field_end[0] == field_begin[0]) throw std::runtime_error(where + "the contig is empty");
		int64_t number_of[2] = { 0, 0 };
		for (int f = 1; f < 3; ++f) {
			if (field_end[f] == field_begin[f]) throw std::runtime_error(where + (f == 1 ? "the start is empty" : "the end is empty"));
			for (size_t k = field_begin[f]; k < field_end[f]; ++k) {
				if (text[k] < '0' || text[k] > '9') throw std::runtime_error(where + (f == 1 ? "the start" : "the end") + " holds something that is not a digit");
				if (number_of[f - 1] <= 0x7FFFFFFFll) number_of[f - 1] = number_of[f - 1] * 10 + (text[k] - '0');
			}
			if (number_of[f - 1] > 0x7FFFFFFFll) throw std::runtime_error(where + (f == 1 ? "the start" : "the end") + " is above 2^31-1");
		}
		if (number_of[0] > number_of[1]) throw std::runtime_error(where + "the start lies behind the end");
		RrnaInterval interval; interval.contig.assign(text, field_begin[0], field_end[0] - field_begin[0]); interval.start = number_of[0]; interval.end = number_of[1];
		intervals.push_back(interval);
	}
}

namespace {
enum { EVENT_R = 0, EVENT_C = 1, EVENT_E = 2, EVENT_GENE_FORWARD = 3, EVENT_GENE_REVERSE = 4, EVENT_KINDS = 5 };
struct Event { int64_t position; int32_t kind, delta; uint32_t gene; };
// [first, last] inclusive, 0-based; what lies before 0 is cut off
void add_events(std::vector<Event>& events, int kind, int64_t first, int64_t last, uint32_t gene) {
	if (first < 0) first = 0;
	if (last < first) return;
	const Event open = { first, kind, +1, gene }, close = { last + 1, kind, -1, gene };
	events.push_back(open); events.push_back(close);
}
std::atomic<uint64_t> g_track_id(0);
}

// n_contigs: the contigs 0 .. n_contigs - 1 of `contigs` get a track (those the session knew when it was opened); genes >= annotation.real_genes are dummies and do not count
void region_track_build(const Annotation& annotation, const Contigs& contigs, size_t n_contigs, const std::vector<RrnaInterval>& intervals, RegionTrack& track) {
	using namespace agpu;
	track = RegionTrack();
	track.id = ++g_track_id;
	const size_t n_genes = annotation.real_genes;
	std::vector<std::vector<Event> > events(n_contigs);
	for (size_t g = 0; g < n_genes; ++g) {
		const GeneRecord& gene = annotation.genes[g];
		if (gene.contig < n_contigs) add_events(events[gene.contig], gene.strand ? EVENT_GENE_FORWARD : EVENT_GENE_REVERSE, gene.start, gene.end, (uint32_t) g);
	}
	for (size_t x = 0; x < annotation.exons.size(); ++x) {
		const ExonRecord& exon = annotation.exons[x];
		if (exon.gene < 0 || (size_t) exon.gene >= n_genes || exon.contig >= n_contigs) continue;
		add_events(events[exon.contig], EVENT_E, exon.start, exon.end, (uint32_t) exon.gene);
		if (exon.coding_region_start != -1) add_events(events[exon.contig], EVENT_C, std::max(exon.start, exon.coding_region_start), std::min(exon.end, exon.coding_region_end), (uint32_t) exon.gene);
	}
	track.intervals = intervals.size();
	for (size_t k = 0; k < intervals.size(); ++k) {
		std::map<std::string, contig_t>::const_iterator known = contigs.by_name.find(remove_chr(intervals[k].contig)); // (the session keeps its names without "chr")
		if (known == contigs.by_name.end() || known->second >= n_contigs) { ++track.intervals_unknown_contig; continue; }
		add_events(events[known->second], EVENT_R, intervals[k].start, intervals[k].end - 1, RNAM_NO_GENE);
	}
	std::vector<uint64_t> rank_so_far(n_genes, 0); // exonic positions of the gene before the sweep line, counted once where its exons overlap
	track.contig_offset.assign(n_contigs + 1, 0);
	for (size_t contig = 0; contig < n_contigs; ++contig) {
		track.contig_offset[contig] = (uint32_t) track.run_start.size();
		std::vector<Event>& list = events[contig];
		std::stable_sort(list.begin(), list.end(), [](const Event& a, const Event& b) { return a.position < b.position; });
		int64_t open[EVENT_KINDS] = { 0, 0, 0, 0, 0 };
		std::map<uint32_t, int64_t> exon_owners; // gene -> its exons over the sweep line
		int64_t from = 0;
		size_t k = 0;
		for (;;) {
			while (k < list.size() && list[k].position <= from) { // (position < from only for position 0 events at the start, which are == from)
				open[list[k].kind] += list[k].delta;
				if (list[k].kind == EVENT_E) { int64_t& count = exon_owners[list[k].gene]; count += list[k].delta; if (count == 0) exon_owners.erase(list[k].gene); }
				++k;
			}
			const int64_t until = k < list.size() ? list[k].position : (int64_t) 0x80000000ll; // the piece [from, until) has one state
			if (from <= 0x7FFFFFFFll) {
				const uint8_t bits = (uint8_t) ((open[EVENT_R] > 0 ? RNAM_BIT_R : 0) | (open[EVENT_C] > 0 ? RNAM_BIT_C : 0) | (open[EVENT_E] > 0 ? RNAM_BIT_E : 0) |
				                                 (open[EVENT_GENE_FORWARD] > 0 ? RNAM_BIT_GENE_FORWARD : 0) | (open[EVENT_GENE_REVERSE] > 0 ? RNAM_BIT_GENE_REVERSE : 0));
				uint32_t gene = RNAM_NO_GENE, rank = 0;
				if (exon_owners.size() == 1) { gene = exon_owners.begin()->first; rank = (uint32_t) rank_so_far[gene]; }
				track.run_start.push_back((int32_t) from); track.run_bits.push_back(bits); track.run_gene.push_back(gene); track.run_rank.push_back(rank);
			}
			if (k >= list.size()) break;
			for (std::map<uint32_t, int64_t>::const_iterator owner = exon_owners.begin(); owner != exon_owners.end(); ++owner) rank_so_far[owner->first] += (uint64_t) (until - from);
			from = until;
		}
	}
	track.contig_offset[n_contigs] = (uint32_t) track.run_start.size();
	// L and strand of every gene; a gene shorter than RNAM_MIN_BODY_LENGTH is nobody's body gene
	track.gene_body.assign(n_genes, 0);
	for (size_t g = 0; g < n_genes; ++g) {
		if (rank_so_far[g] > 0x7FFFFFFFull) throw std::runtime_error("region track: a gene with more than 2^31-1 exonic bases");
		track.gene_body[g] = (uint32_t) rank_so_far[g] | (annotation.genes[g].strand ? RNAM_FORWARD_GENE : 0u);
	}
	// neighbouring runs with equal bits and equal body gene are one run
	size_t kept = 0;
	for (size_t contig = 0; contig < n_contigs; ++contig) {
		const size_t begin = track.contig_offset[contig], end = track.contig_offset[contig + 1];
		track.contig_offset[contig] = (uint32_t) kept;
		for (size_t r = begin; r < end; ++r) {
			uint32_t gene = track.run_gene[r], rank = track.run_rank[r];
			if (gene != RNAM_NO_GENE && (track.gene_body[gene] & ~RNAM_FORWARD_GENE) < RNAM_MIN_BODY_LENGTH) { gene = RNAM_NO_GENE; }
			if (gene == RNAM_NO_GENE) rank = 0;
			if (kept > track.contig_offset[contig] && track.run_bits[kept - 1] == track.run_bits[r] && track.run_gene[kept - 1] == gene) continue;
			track.run_start[kept] = track.run_start[r]; track.run_bits[kept] = track.run_bits[r]; track.run_gene[kept] = gene; track.run_rank[kept] = rank;
			++kept;
		}
	}
	track.contig_offset[n_contigs] = (uint32_t) kept;
	track.run_start.resize(kept); track.run_bits.resize(kept); track.run_gene.resize(kept); track.run_rank.resize(kept);
	if (track.run_start.size() >= 0xFFFFFFF0ull) throw std::runtime_error("region track: more than 2^32-16 runs");
}

}
