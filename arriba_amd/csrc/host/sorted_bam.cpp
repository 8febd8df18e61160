// arriba_amd/csrc/host/sorted_bam.cpp -- the host side of --sorted-bam (include/arriba_host.h: ahost_sorted_bam_*): the header of the output (the input's, with
// "@HD ... SO:coordinate"), arriba_amd/csrc/device/sorted_bam_core.hpp stepped on the host over records in host memory (key, std::stable_sort, offsets, framing, index: the
// comparator of agpu_sorted_bam.hip, and what --host-ingest and the CPU tier run), and the writer of FILE.bai (SAMv1 5.2).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>
#include "arriba_host.h"
#include "../device/crc32_core.hpp"
#include "../device/sorted_bam_core.hpp"
#include "../device/deflate_out_core.hpp"
#include "../device/markdup_core.hpp"

namespace arriba {

namespace {

const agpu::Crc32Tables& crc_tables() { static agpu::Crc32Tables tables; static bool made = false; if (!made) { agpu::crc32_make_tables(tables); made = true; } return tables; }
void put32(std::vector<uint8_t>& out, uint32_t v) { for (int k = 0; k < 4; ++k) out.push_back((uint8_t) (v >> (8 * k))); }
void put64(std::vector<uint8_t>& out, uint64_t v) { for (int k = 0; k < 8; ++k) out.push_back((uint8_t) (v >> (8 * k))); }
uint32_t get32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }

// the first line of the header text says SO:coordinate (and only that sort order)
std::string with_coordinate_order(const std::string& text) {
	if (text.compare(0, 3, "@HD") != 0 || (text.size() > 3 && text[3] != '\t' && text[3] != '\n')) return "@HD\tVN:1.6\tSO:coordinate\n" + text;
	size_t line_end = text.find('\n');
	if (line_end == std::string::npos) line_end = text.size();
	std::string line = text.substr(0, line_end), rest = text.substr(line_end), carriage;
	if (!line.empty() && line[line.size() - 1] == '\r') { line.erase(line.size() - 1); carriage = "\r"; }
	std::string out; bool placed = false;
	for (size_t field = 0; field <= line.size(); ) {
		size_t field_end = line.find('\t', field);
		if (field_end == std::string::npos) field_end = line.size();
		const bool sort_order = line.compare(field, 3, "SO:") == 0;
		if (!sort_order || !placed) { if (field > 0) out += '\t'; out += sort_order ? std::string("SO:coordinate") : line.substr(field, field_end - field); }
		if (sort_order) placed = true;
		field = field_end + 1;
	}
	if (!placed) out += "\tSO:coordinate";
	return out + carriage + rest;
}

}

// input: the head of the uncompressed input, either a BAM header (magic ... the last reference) or the '@' lines of SAM text -> the BAM header of the sorted file
void sorted_bam_header(const uint8_t* input, size_t size, std::vector<uint8_t>& out, std::vector<uint32_t>& ref_length) {
	std::string text; std::vector<std::string> names; ref_length.clear();
	if (size >= 4 && memcmp(input, "BAM\1", 4) == 0) {
		if (size < 12) throw std::runtime_error("failed to read SAM header");
		const uint64_t l_text = get32(input + 4);
		if (size < 12 + l_text) throw std::runtime_error("failed to read SAM header");
		text.assign((const char*) input + 8, l_text);
		const uint32_t n_ref = get32(input + 8 + l_text);
		uint64_t at = 12 + l_text;
		for (uint32_t t = 0; t < n_ref; ++t) {
			if (size < at + 4) throw std::runtime_error("failed to read SAM header");
			const uint64_t l_name = get32(input + at);
			if (size < at + 4 + l_name + 4) throw std::runtime_error("failed to read SAM header");
			names.push_back(std::string((const char*) input + at + 4, l_name > 0 ? l_name - 1 : 0));
			ref_length.push_back(get32(input + at + 4 + l_name));
			at += 8 + l_name;
		}
	} else {
		size_t at = 0; uint64_t line_number = 0;
		while (at < size && input[at] == '@') {
			const uint8_t* feed = (const uint8_t*) memchr(input + at, '\n', size - at);
			size_t end = feed != NULL ? (size_t) (feed - input) : size;
			const size_t next = feed != NULL ? end + 1 : size;
			if (end > at && input[end - 1] == '\r') --end;
			const std::string line((const char*) input + at, end - at);
			++line_number;
			if (line.compare(0, 4, "@SQ\t") == 0) {
				std::string name; bool has_length = false; uint64_t length = 0;
				for (size_t field = 4; field < line.size(); ) {
					size_t field_end = line.find('\t', field);
					if (field_end == std::string::npos) field_end = line.size();
					if (line.compare(field, 3, "SN:") == 0) name = line.substr(field + 3, field_end - field - 3);
					else if (line.compare(field, 3, "LN:") == 0 && field_end > field + 3) { has_length = true; length = strtoull(line.c_str() + field + 3, NULL, 10); }
					field = field_end + 1;
				}
				if (name.empty()) throw std::runtime_error("SAM header line " + std::to_string(line_number) + ": @SQ without SN");
				if (!has_length) throw std::runtime_error("SAM header line " + std::to_string(line_number) + ": @SQ without LN");
				names.push_back(name); ref_length.push_back((uint32_t) length);
			}
			at = next;
		}
		text.assign((const char*) input, at);
		if (!text.empty() && text[text.size() - 1] != '\n') text += '\n';
	}
	text = with_coordinate_order(text);
	out.assign({ 'B', 'A', 'M', 1 });
	put32(out, (uint32_t) text.size()); out.insert(out.end(), text.begin(), text.end());
	put32(out, (uint32_t) names.size());
	for (size_t t = 0; t < names.size(); ++t) { put32(out, (uint32_t) names[t].size() + 1); out.insert(out.end(), names[t].begin(), names[t].end()); out.push_back(0); put32(out, ref_length[t]); }
}

// bytes -> stored BGZF blocks of SBAM_PAYLOAD bytes (the last one shorter), appended to `out`
void sorted_bam_frame(const uint8_t* bytes, uint64_t size, std::vector<uint8_t>& out) {
	const agpu::Crc32Tables& tables = crc_tables();
	for (uint64_t at = 0; at < size; at += agpu::SBAM_PAYLOAD) {
		const uint32_t n = (uint32_t) std::min<uint64_t>(agpu::SBAM_PAYLOAD, size - at);
		for (uint32_t i = 0; i < agpu::SBAM_HEAD; ++i) out.push_back(agpu::sbam_head_byte(i, n));
		out.insert(out.end(), bytes + at, bytes + at + n);
		const uint32_t crc = agpu::crc32_of_sliced(tables.slice, bytes + at, n);
		for (uint32_t i = 0; i < agpu::SBAM_TAIL; ++i) out.push_back(agpu::sbam_tail_byte(i, crc, n));
	}
}

namespace {

// deflate_out_core.hpp stepped on the host over one payload: the rounds of the device (64 lanes whose loads of a round all come before its stores, a table per segment), the
// histograms, the codes, the bits.  The BGZF block is appended to `out`; a payload that no encoding makes smaller comes out as the stored block of sorted_bam_frame.
void deflated_block(const uint8_t* payload, uint32_t n, std::vector<uint8_t>& out) {
	using namespace agpu;
	std::vector<uint32_t> token(n, 0);
	for (uint32_t segment_begin = 0; segment_begin < n; segment_begin += DFO_SEGMENT) {
		const uint32_t segment_end = dfo_segment_end(segment_begin, n);
		uint32_t table[DFO_HASH_SLOTS] = { 0 };
		uint32_t next = segment_begin; // the first position that no token covers yet
		for (uint32_t base = segment_begin; base < segment_end; base += DFO_ROUND) {
			const uint32_t count = std::min(DFO_ROUND, segment_end - base);
			const bool covered = next >= base + count; // (a match reaches over the whole round: nothing is looked up, the positions are entered all the same)
			uint32_t found[DFO_ROUND];
			if (!covered) for (uint32_t lane = 0; lane < count; ++lane) {
				const uint32_t p = base + lane;
				const bool hashable = dfo_hashable(p, segment_end);
				const uint32_t value = hashable ? dfo_load32(payload, p) : 0;
				found[lane] = dfo_find(payload, p, segment_end, hashable ? table[dfo_hash(value)] : 0, value);
			}
			for (uint32_t lane = 0; lane < count; ++lane) {
				const uint32_t p = base + lane;
				if (dfo_hashable(p, segment_end)) { uint32_t& slot = table[dfo_hash(dfo_load32(payload, p))]; slot = std::max(slot, p + 1); }
			}
			if (!covered) {
				uint32_t at = std::max(next, base);
				while (at < base + count) { token[at] = found[at - base]; at += dfo_token_span(found[at - base]); }
				next = at;
			}
		}
	}
	DfoState s; memset(&s, 0, sizeof(s));
	s.ll_count[DFO_END] = 1;
	for (uint32_t p = 0; p < n; ++p) if (token[p] != 0) {
		uint32_t ll, d, extra;
		dfo_token_symbols(token[p], ll, d, extra);
		++s.ll_count[ll]; if (d < DFO_D) ++s.d_count[d]; s.extra_bits += extra;
	}
	for (uint32_t t = 0; t < DFO_LL; ++t) if (s.ll_count[t] != 0) { s.ll_sorted[dfo_rank(s.ll_count, DFO_LL, t)] = (uint16_t) t; ++s.ll_used; }
	for (uint32_t t = 0; t < DFO_D; ++t) if (s.d_count[t] != 0) { s.d_sorted[dfo_rank(s.d_count, DFO_D, t)] = (uint16_t) t; ++s.d_used; }
	dfo_plan_lengths(s);
	for (uint32_t t = 0; t < DFO_CL; ++t) if (s.cl_count[t] != 0) { s.cl_sorted[dfo_rank(s.cl_count, DFO_CL, t)] = (uint16_t) t; ++s.cl_used; }
	dfo_plan(s, n);
	if (s.btype == DFO_STORED) { sorted_bam_frame(payload, n, out); return; }
	for (uint32_t t = 0; t < DFO_LL; ++t) s.ll_code[t] = (uint16_t) dfo_code_of(s.ll_length, s.ll_first, t);
	for (uint32_t t = 0; t < DFO_D; ++t) s.d_code[t] = (uint16_t) dfo_code_of(s.d_length, s.d_first, t);
	for (uint32_t t = 0; t < DFO_CL; ++t) s.cl_code[t] = (uint16_t) dfo_code_of(s.cl_length, s.cl_first, t);
	std::vector<uint32_t> words((s.total_bits + 31) / 32 + 2, 0);
	const auto or_word = [&words](uint32_t word, uint32_t bits) { words[word] |= bits; };
	dfo_put_header(s, 0, or_word);
	uint64_t at = s.header_bits;
	for (uint32_t p = 0; p < n; ++p) if (token[p] != 0) { dfo_put_token(s, at, token[p], or_word); at += dfo_token_bits(s, token[p]); }
	dfo_put(at, dfo_end_value(s), dfo_end_bits(s), or_word); at += dfo_end_bits(s);
	if (at != s.total_bits) throw std::runtime_error("deflate: the bits of a block do not add up to their count");
	const uint32_t data_bytes = (s.total_bits + 7) / 8, bsize = dfo_block_bytes(s.total_bits) - 1;
	for (uint32_t i = 0; i < 16; ++i) out.push_back(sbam_head_byte(i, n));
	out.push_back((uint8_t) bsize); out.push_back((uint8_t) (bsize >> 8));
	for (uint32_t i = 0; i < data_bytes; ++i) out.push_back((uint8_t) (words[i / 4] >> (8 * (i % 4))));
	const uint32_t crc = crc32_of_sliced(crc_tables().slice, payload, n);
	for (uint32_t i = 0; i < SBAM_TAIL; ++i) out.push_back(sbam_tail_byte(i, crc, n));
}

}

// the same at a compression level (0: stored, 1: deflate_out_core.hpp); block_offset: where every block begins in `out`, counted from first_offset, one entry more for the end
void sorted_bam_frame_level(const uint8_t* bytes, uint64_t size, int level, std::vector<uint8_t>& out, uint64_t first_offset, std::vector<uint64_t>& block_offset) {
	const size_t base = out.size();
	block_offset.clear();
	for (uint64_t at = 0; at < size; at += agpu::SBAM_PAYLOAD) {
		const uint32_t n = (uint32_t) std::min<uint64_t>(agpu::SBAM_PAYLOAD, size - at);
		block_offset.push_back(first_offset + (out.size() - base));
		if (level == 0) sorted_bam_frame(bytes + at, n, out); else deflated_block(bytes + at, n, out);
	}
	block_offset.push_back(first_offset + (out.size() - base));
}

agpu_sorted_bam_index_arrays SortedBam::view(uint32_t n_ref) {
	agpu_sorted_bam_index_arrays v; memset(&v, 0, sizeof(v));
	v.n_ref = n_ref; v.n_chunks = chunk_key.size(); v.n_intervals = intervals.size(); v.n_no_coor = n_no_coor;
	v.chunk_key = chunk_key.data(); v.chunk_begin = chunk_begin.data(); v.chunk_end = chunk_end.data(); v.interval_offset = interval_offset.data(); v.intervals = intervals.data();
	v.ref_begin = ref_begin.data(); v.ref_end = ref_end.data(); v.ref_mapped = ref_mapped.data(); v.ref_unmapped = ref_unmapped.data();
	return v;
}

bool references_fit_bai(const uint32_t* ref_length, uint32_t n_ref) { for (uint32_t t = 0; t < n_ref; ++t) if (ref_length[t] > (uint32_t) agpu::SBAM_MAX_REFERENCE) return false; return true; }

// ref_length == NULL: no index
// duplicate (--mark-duplicates; NULL: the records as they are): one byte per record of the input, markdup_flags' -- bit 0x400 of every record is set or cleared by it in the copy
void sorted_bam_of(const uint8_t* records, uint64_t size, uint64_t first_block_file_offset, const uint32_t* ref_length, uint32_t n_ref, SortedBam& result, int level, const uint8_t* duplicate) {
	using namespace agpu;
	if (level != 0 && level != 1) throw std::runtime_error("the compression level of a sorted BAM file is 0 (stored) or 1");
	// the record chain
	std::vector<uint64_t> offset;
	for (uint64_t at = 0; at < size; ) {
		if (size - at < 36 || (uint64_t) get32(records + at) + 4 > size - at || get32(records + at) < 32) throw std::runtime_error("failed to load alignments");
		offset.push_back(at);
		at += (uint64_t) get32(records + at) + 4;
	}
	const uint64_t n = offset.size();
	if (n >= 0xFFFFFFF0ull) throw std::runtime_error("more than 2^32-16 alignment records");
	std::vector<SbamRecord> parsed(n);
	for (uint64_t r = 0; r < n; ++r) parsed[r] = sbam_parse(records, offset[r], size);
	std::vector<uint32_t> order(n);
	for (uint64_t r = 0; r < n; ++r) order[r] = (uint32_t) r;
	std::stable_sort(order.begin(), order.end(), [&parsed](uint32_t a, uint32_t b) { return parsed[a].key < parsed[b].key; });
	std::vector<uint64_t> out_offset(n + 1, 0);
	for (uint64_t i = 0; i < n; ++i) out_offset[i + 1] = out_offset[i] + parsed[order[i]].size;
	// gather and frame
	std::vector<uint8_t> sorted(size);
	for (uint64_t i = 0; i < n; ++i) memcpy(sorted.data() + out_offset[i], records + offset[order[i]], parsed[order[i]].size);
	if (duplicate != NULL) for (uint64_t i = 0; i < n; ++i) { uint8_t& byte = sorted[out_offset[i] + MDUP_FLAG_BYTE]; byte = (uint8_t) ((byte & ~MDUP_FLAG_MASK) | (duplicate[order[i]] != 0 ? MDUP_FLAG_MASK : 0u)); }
	result.blocks.clear(); result.blocks.reserve(size + sbam_block_count(size) * (SBAM_HEAD + SBAM_TAIL));
	std::vector<uint64_t> block_offset;
	sorted_bam_frame_level(sorted.data(), size, level, result.blocks, first_block_file_offset, block_offset);
	memset(&result.info, 0, sizeof(result.info));
	result.info.records = n; result.info.uncompressed_bytes = size; result.info.file_bytes = result.blocks.size(); result.info.windows = size > 0 ? 1 : 0; result.info.window_bytes = result.blocks.size();
	// the index
	result.indexed = ref_length != NULL;
	if (!result.indexed) return;
	sorted_bam_index_of(n, [&](uint64_t i) {
		const SbamRecord& r = parsed[order[i]];
		if (level != 0) { const SortedBamIndexed record = { r.ref, r.pos, r.end, (r.flag & 4u) != 0, sbam_voffset(block_offset.data(), out_offset[i]), sbam_voffset(block_offset.data(), out_offset[i + 1]) }; return record; }
		const SortedBamIndexed record = { r.ref, r.pos, r.end, (r.flag & 4u) != 0, sbam_voffset(first_block_file_offset, out_offset[i]), sbam_voffset(first_block_file_offset, out_offset[i + 1]) };
		return record;
	}, ref_length, n_ref, result);
}

// the arrays of the index from the records of a file in file order (what the kernels of agpu_sorted_bam.hip compute; --supporting-alignments makes the indexes of its small files here)
void sorted_bam_index_of(uint64_t n, const std::function<SortedBamIndexed(uint64_t)>& record, const uint32_t* ref_length, uint32_t n_ref, SortedBam& result) {
	using namespace agpu;
	result.indexed = true;
	if (!references_fit_bai(ref_length, n_ref)) throw std::runtime_error("a reference is longer than 2^29 bases: a BAI index cannot address it");
	result.interval_offset.assign((size_t) n_ref + 1, 0);
	for (uint32_t t = 0; t < n_ref; ++t) result.interval_offset[t + 1] = result.interval_offset[t] + sbam_windows_of(ref_length[t]);
	result.intervals.assign(result.interval_offset[n_ref], SBAM_NO_OFFSET);
	result.ref_begin.assign(n_ref, SBAM_NO_OFFSET); result.ref_end.assign(n_ref, 0); result.ref_mapped.assign(n_ref, 0); result.ref_unmapped.assign(n_ref, 0);
	result.n_no_coor = 0;
	std::vector<uint64_t> run_key, run_begin, run_end;
	bool open = false;
	for (uint64_t i = 0; i < n; ++i) {
		const SortedBamIndexed r = record(i);
		const uint64_t begin = r.begin_offset, end = r.end_offset;
		if (r.ref < 0) ++result.n_no_coor;
		else if ((uint32_t) r.ref < n_ref) {
			result.ref_begin[r.ref] = std::min(result.ref_begin[r.ref], begin); result.ref_end[r.ref] = std::max(result.ref_end[r.ref], end);
			++(r.unmapped ? result.ref_unmapped : result.ref_mapped)[r.ref];
		}
		if (!sbam_indexed(r.ref, r.pos, n_ref)) { open = false; continue; }
		const uint64_t key = sbam_chunk_key(r.ref, sbam_reg2bin(r.pos, r.end));
		if (!open || run_key.back() != key) { run_key.push_back(key); run_begin.push_back(begin); run_end.push_back(end); open = true; }
		else run_end.back() = end;
		uint64_t first, last;
		if (sbam_window_range(r.pos, r.end, sbam_windows_of(ref_length[r.ref]), first, last))
			for (uint64_t w = first; w <= last; ++w) { uint64_t& slot = result.intervals[result.interval_offset[r.ref] + w]; slot = std::min(slot, begin); }
	}
	for (uint32_t t = 0; t < n_ref; ++t) {
		if (result.ref_begin[t] == SBAM_NO_OFFSET) result.ref_begin[t] = 0;
		uint64_t next = 0;
		for (uint64_t w = result.interval_offset[t + 1]; w-- > result.interval_offset[t]; ) { if (result.intervals[w] == SBAM_NO_OFFSET) result.intervals[w] = next; else next = result.intervals[w]; }
	}
	std::vector<uint32_t> chunk_order(run_key.size());
	for (size_t c = 0; c < chunk_order.size(); ++c) chunk_order[c] = (uint32_t) c;
	std::stable_sort(chunk_order.begin(), chunk_order.end(), [&run_key](uint32_t a, uint32_t b) { return run_key[a] < run_key[b]; });
	result.chunk_key.resize(run_key.size()); result.chunk_begin.resize(run_key.size()); result.chunk_end.resize(run_key.size());
	for (size_t c = 0; c < chunk_order.size(); ++c) { result.chunk_key[c] = run_key[chunk_order[c]]; result.chunk_begin[c] = run_begin[chunk_order[c]]; result.chunk_end[c] = run_end[chunk_order[c]]; }
}

// FILE.bai from the finished arrays (SAMv1 5.2): per reference its bins with their chunks, the pseudo-bin 37450, the linear index up to the last window that has a record
void sorted_bam_bai(const agpu_sorted_bam_index_arrays& index, std::vector<uint8_t>& out) {
	out.assign({ 'B', 'A', 'I', 1 });
	put32(out, index.n_ref);
	uint64_t c = 0;
	for (uint32_t t = 0; t < index.n_ref; ++t) {
		const uint64_t first = c;
		uint32_t n_bins = 0;
		for (uint64_t k = c; k < index.n_chunks && index.chunk_key[k] >> 32 == t; ++k) if (k == c || index.chunk_key[k] != index.chunk_key[k - 1]) ++n_bins;
		const bool has_records = index.ref_mapped[t] + index.ref_unmapped[t] > 0;
		put32(out, n_bins + (has_records ? 1 : 0));
		while (c < index.n_chunks && index.chunk_key[c] >> 32 == t) {
			uint64_t run = c;
			while (run < index.n_chunks && index.chunk_key[run] == index.chunk_key[c]) ++run;
			put32(out, (uint32_t) index.chunk_key[c]); put32(out, (uint32_t) (run - c));
			for (; c < run; ++c) { put64(out, index.chunk_begin[c]); put64(out, index.chunk_end[c]); }
		}
		(void) first;
		if (has_records) { put32(out, agpu::SBAM_PSEUDO_BIN); put32(out, 2); put64(out, index.ref_begin[t]); put64(out, index.ref_end[t]); put64(out, index.ref_mapped[t]); put64(out, index.ref_unmapped[t]); }
		uint64_t n_intv = index.interval_offset[t + 1] - index.interval_offset[t];
		while (n_intv > 0 && index.intervals[index.interval_offset[t] + n_intv - 1] == 0) --n_intv;
		put32(out, (uint32_t) n_intv);
		for (uint64_t w = 0; w < n_intv; ++w) put64(out, index.intervals[index.interval_offset[t] + w]);
	}
	put64(out, index.n_no_coor);
}

void write_file(const std::string& path, const std::vector<const std::vector<uint8_t>*>& parts) {
	FILE* file = fopen(path.c_str(), "wb");
	if (file == NULL) throw std::runtime_error("failed to open '" + path + "' for writing");
	bool good = true;
	for (size_t k = 0; k < parts.size() && good; ++k) good = parts[k]->empty() || fwrite(parts[k]->data(), 1, parts[k]->size(), file) == parts[k]->size();
	if (fclose(file) != 0) good = false;
	if (!good) { remove(path.c_str()); throw std::runtime_error("failed to write '" + path + "'"); }
}

// the whole output on the host: FILE and FILE.bai through FILE.tmp / FILE.bai.tmp
void sorted_bam_write(const uint8_t* input_header, size_t header_size, const uint8_t* records, uint64_t size, const std::string& path, agpu_sorted_bam_info* info, int level, bool mark_duplicates, agpu_markdup_counts* counts) {
	if (level != 0 && level != 1) throw std::runtime_error("the compression level of a sorted BAM file is 0 (stored) or 1");
	std::vector<uint8_t> header, framed_header, bai, eof; std::vector<uint32_t> ref_length;
	sorted_bam_header(input_header, header_size, header, ref_length);
	sorted_bam_frame(header.data(), header.size(), framed_header);
	for (uint32_t i = 0; i < agpu::SBAM_EOF_BYTES; ++i) eof.push_back(agpu::sbam_eof_byte(i));
	const bool with_index = references_fit_bai(ref_length.data(), (uint32_t) ref_length.size());
	if (!with_index) std::cerr << "WARNING: a reference is longer than 2^29 bases, which a BAI index cannot address: '" << path << "' is written without '" << path << ".bai'" << std::endl;
	SortedBam sorted;
	std::vector<uint8_t> duplicate; agpu_markdup_counts counted; memset(&counted, 0, sizeof(counted));
	if (mark_duplicates) markdup_flags(records, size, duplicate, counted);
	if (counts) *counts = counted;
	sorted_bam_of(records, size, framed_header.size(), with_index ? ref_length.data() : NULL, (uint32_t) ref_length.size(), sorted, level, mark_duplicates ? duplicate.data() : NULL);
	const std::string bam_tmp = path + ".tmp", bai_tmp = path + ".bai.tmp";
	try {
		write_file(bam_tmp, { &framed_header, &sorted.blocks, &eof });
		if (with_index) { const agpu_sorted_bam_index_arrays view = sorted.view((uint32_t) ref_length.size()); sorted_bam_bai(view, bai); write_file(bai_tmp, { &bai }); }
		if (rename(bam_tmp.c_str(), path.c_str()) != 0) throw std::runtime_error("failed to write '" + path + "'");
		if (with_index && rename(bai_tmp.c_str(), (path + ".bai").c_str()) != 0) throw std::runtime_error("failed to write '" + path + ".bai'");
	} catch (...) { remove(bam_tmp.c_str()); remove(bai_tmp.c_str()); throw; }
	if (info) *info = sorted.info;
}

}
