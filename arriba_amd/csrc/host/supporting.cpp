// arriba_amd/csrc/host/supporting.cpp -- the host side of --supporting-alignments (include/arriba_host.h: ahost_supporting_*): the writer that cuts the framed record blocks
// of all rows into the files PREFIX_ID.bam / PREFIX_ID.bam.bai (the blocks come from the device, or from the stepping below), the indexes of those small files from the arrays
// of their records (the index builder of sorted_bam.cpp), and arriba_amd/csrc/device/supporting_core.hpp stepped on the host over records in host memory: name table, marks,
// pool in coordinate order, join with the rows, emissions, framing -- the comparator of agpu_supporting.hip, and what --host-ingest and the CPU tier run.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>
#include "arriba_host.h"
#include "../device/supporting_core.hpp"

namespace arriba {

namespace {
uint32_t get32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
}

// ---- the writer ----

std::string SupportingWriter::path_of(uint32_t row) const { return prefix_ + "_" + std::to_string(row + 1) + ".bam"; }

SupportingWriter::SupportingWriter(const std::string& prefix, const uint8_t* framed_header, uint64_t framed_bytes, uint32_t n_rows, const uint64_t* row_file_bytes)
	: prefix_(prefix), header_(framed_header, framed_header + framed_bytes), row_bytes_(row_file_bytes, row_file_bytes + n_rows), row_(0), written_(0), file_(NULL), indexed_(false) {}

SupportingWriter::~SupportingWriter() { abandon(); }

void SupportingWriter::open_row() {
	const std::string path = path_of(row_) + ".tmp";
	file_ = fopen(path.c_str(), "wb");
	if (file_ == NULL) throw std::runtime_error("failed to open '" + path + "' for writing");
	temporaries_.push_back(path);
	if (!header_.empty() && fwrite(header_.data(), 1, header_.size(), file_) != header_.size()) throw std::runtime_error("failed to write '" + path + "'");
	written_ = 0;
}

void SupportingWriter::close_row() {
	uint8_t eof[agpu::SBAM_EOF_BYTES];
	for (uint32_t i = 0; i < agpu::SBAM_EOF_BYTES; ++i) eof[i] = agpu::sbam_eof_byte(i);
	const bool written = fwrite(eof, 1, sizeof(eof), file_) == sizeof(eof);
	const int closed = fclose(file_); file_ = NULL;
	if (!written || closed != 0) throw std::runtime_error("failed to write '" + path_of(row_) + ".tmp'");
	++row_;
}

// rows without a record are written as they are reached: header and end-of-file block
void SupportingWriter::skip_finished_rows() {
	while (row_ < row_bytes_.size() && (file_ != NULL ? written_ == row_bytes_[row_] : row_bytes_[row_] == 0)) {
		if (file_ == NULL) open_row();
		close_row();
	}
}

void SupportingWriter::push(const uint8_t* bytes, uint64_t size) {
	while (size > 0) {
		skip_finished_rows();
		if (row_ >= row_bytes_.size()) throw std::runtime_error("more record blocks than the rows of '" + prefix_ + "' hold");
		if (file_ == NULL) open_row();
		const uint64_t take = std::min<uint64_t>(size, row_bytes_[row_] - written_);
		if (fwrite(bytes, 1, take, file_) != take) throw std::runtime_error("failed to write '" + path_of(row_) + ".tmp'");
		written_ += take; bytes += take; size -= take;
	}
	skip_finished_rows();
}

// PREFIX_ID.bam.bai.tmp of every row from the arrays of the records of all files; a reference longer than 2^29 bases: no index, and the warning of --sorted-bam
void SupportingWriter::index(const agpu_supporting_index_arrays& arrays, const uint32_t* ref_length, uint32_t n_ref) {
	if (arrays.n_rows != row_bytes_.size()) throw std::runtime_error("the index arrays are not those of the rows of '" + prefix_ + "'");
	if (!references_fit_bai(ref_length, n_ref)) {
		std::cerr << "WARNING: a reference is longer than 2^29 bases, which a BAI index cannot address: the files '" << prefix_ << "_*.bam' are written without '.bai'" << std::endl;
		return;
	}
	for (uint32_t row = 0; row < arrays.n_rows; ++row) {
		const uint64_t first = arrays.row_first[row], n = arrays.row_first[row + 1] - first;
		SortedBam result;
		sorted_bam_index_of(n, [&](uint64_t i) {
			const uint64_t e = first + i;
			const SortedBamIndexed record = { arrays.ref[e], arrays.pos[e], (int32_t) (arrays.end_flag[e] & 0x7FFFFFFFu), (arrays.end_flag[e] >> 31) != 0, arrays.begin[e], arrays.end[e] };
			return record;
		}, ref_length, n_ref, result);
		std::vector<uint8_t> bai;
		const agpu_sorted_bam_index_arrays view = result.view(n_ref);
		sorted_bam_bai(view, bai);
		const std::string path = path_of(row) + ".bai.tmp";
		temporaries_.push_back(path);
		write_file(path, { &bai });
	}
	indexed_ = true;
}

// every file is complete: the temporaries take their names
void SupportingWriter::commit() {
	skip_finished_rows();
	if (row_ != row_bytes_.size() || file_ != NULL) throw std::runtime_error("the record blocks of '" + prefix_ + "' do not have the size that was announced");
	for (size_t k = 0; k < temporaries_.size(); ++k) {
		const std::string path = temporaries_[k].substr(0, temporaries_[k].size() - 4);
		if (rename(temporaries_[k].c_str(), path.c_str()) != 0) throw std::runtime_error("failed to write '" + path + "'");
		finals_.push_back(path); temporaries_[k].clear();
	}
	temporaries_.clear(); finals_.clear();
}

// nothing of the prefix is left behind
void SupportingWriter::abandon() {
	if (file_ != NULL) { fclose(file_); file_ = NULL; }
	for (size_t k = 0; k < temporaries_.size(); ++k) if (!temporaries_[k].empty()) remove(temporaries_[k].c_str());
	for (size_t k = 0; k < finals_.size(); ++k) remove(finals_[k].c_str());
	temporaries_.clear(); finals_.clear();
}

// ---- the stepping on the host ----

void supporting_alignments(const uint8_t* input_header, size_t header_size, const uint8_t* records, uint64_t size, const char* names, const uint64_t* name_offset, uint64_t n_names, bool strip_hit_index,
                           const agpu_supporting_rows& rows, int64_t window, const std::string& prefix, agpu_supporting_info* info) {
	using namespace agpu;
	if (window < 0 || window > 0x7FFFFFFF) throw std::runtime_error("the window must lie in 0 .. 2^31-1");
	if (n_names >= SUPPORT_MAX_NAMES) throw std::runtime_error("too many names");
	std::vector<uint8_t> header, framed_header; std::vector<uint32_t> ref_length;
	sorted_bam_header(input_header, header_size, header, ref_length);
	sorted_bam_frame(header.data(), header.size(), framed_header);
	// the record chain, the name table, the marks
	std::vector<uint64_t> offset;
	for (uint64_t at = 0; at < size; ) {
		if (size - at < 36 || (uint64_t) get32(records + at) + 4 > size - at || get32(records + at) < 32) throw std::runtime_error("failed to load alignments");
		offset.push_back(at);
		at += (uint64_t) get32(records + at) + 4;
	}
	uint32_t hash_bits = 64;
	if (const char* knob = getenv("ARRIBA_SUPPORT_HASH_BITS")) { const long bits = strtol(knob, NULL, 10); if (bits >= 1 && bits < 64) hash_bits = (uint32_t) bits; }
	const uint64_t no_offsets[1] = { 0 };
	const SupportNames view = { (const uint8_t*) names, n_names > 0 ? name_offset : no_offsets, n_names, strip_hit_index };
	const uint64_t slots = support_table_slots(n_names);
	std::vector<unsigned long long> table(slots, 0);
	std::vector<uint32_t> name_id(n_names);
	for (uint64_t i = 0; i < n_names; ++i) name_id[i] = support_insert(table.data(), slots, view, (uint32_t) i, hash_bits);
	struct Pooled { SbamRecord record; uint64_t at; uint32_t name; };
	std::vector<Pooled> pool;
	for (size_t r = 0; r < offset.size(); ++r) {
		const SbamRecord record = sbam_parse(records, offset[r], size);
		const uint8_t* name; uint32_t length;
		if (record.ref < 0 || !support_qname(records, offset[r], record.size, name, length)) continue;
		const uint32_t id = support_lookup(table.data(), slots, view, name, length, hash_bits);
		if (id != SUPPORT_NONE) { const Pooled pooled = { record, offset[r], id }; pool.push_back(pooled); }
	}
	std::stable_sort(pool.begin(), pool.end(), [](const Pooled& a, const Pooled& b) { return a.record.key < b.record.key; });
	if (pool.size() >= 0xFFFFFFF0ull) throw std::runtime_error("more than 2^32-16 alignment records");
	// (name id, row) grouped by name id; per pooled record the rows of its name and their windows; (row, pool rank) in file order
	const uint32_t n_rows = rows.n_rows;
	std::vector<uint64_t> pairs;
	for (uint32_t row = 0; row < n_rows; ++row)
		for (uint64_t k = rows.name_begin[row]; k < rows.name_begin[row + 1]; ++k) {
			if (rows.names[k] >= n_names) throw std::runtime_error("a row lists a name that is not among the names");
			pairs.push_back(support_pair_key(name_id[rows.names[k]], row));
		}
	std::sort(pairs.begin(), pairs.end());
	std::vector<uint64_t> emissions;
	for (size_t i = 0; i < pool.size(); ++i) {
		const SbamRecord& record = pool[i].record;
		const size_t first = (size_t) (std::lower_bound(pairs.begin(), pairs.end(), support_pair_key(pool[i].name, 0)) - pairs.begin());
		for (size_t k = first; k < pairs.size() && (uint32_t) (pairs[k] >> 32) == pool[i].name; ++k) {
			if (k > first && pairs[k - 1] == pairs[k]) continue;
			const uint32_t row = (uint32_t) pairs[k];
			if (support_overlaps(record.ref, record.pos, record.end, rows.ref[2 * (size_t) row], rows.breakpoint[2 * (size_t) row], window) ||
			    support_overlaps(record.ref, record.pos, record.end, rows.ref[2 * (size_t) row + 1], rows.breakpoint[2 * (size_t) row + 1], window)) emissions.push_back((uint64_t) row << 32 | i);
		}
	}
	std::sort(emissions.begin(), emissions.end());
	// the bytes of every row, framed; the arrays of the index
	const size_t n = emissions.size();
	std::vector<uint64_t> row_first((size_t) n_rows + 1, n), row_file_bytes(n_rows, 0), begin(n), end(n);
	std::vector<int32_t> ref(n), pos(n); std::vector<uint32_t> end_flag(n), bin(n);
	std::vector<uint8_t> framed, payload;
	uint64_t uncompressed = 0, blocks = 0;
	for (size_t e = 0, row = 0; row < n_rows; ++row) {
		row_first[row] = e;
		payload.clear();
		const size_t framed_before = framed.size();
		for (; e < n && emissions[e] >> 32 == row; ++e) {
			const Pooled& pooled = pool[(uint32_t) emissions[e]];
			ref[e] = pooled.record.ref; pos[e] = pooled.record.pos; end_flag[e] = (uint32_t) pooled.record.end | ((pooled.record.flag & 4u) ? 0x80000000u : 0u);
			bin[e] = (pooled.record.pos >= 0 && pooled.record.pos < SBAM_MAX_REFERENCE) ? sbam_reg2bin(pooled.record.pos, pooled.record.end) : SUPPORT_NONE;
			begin[e] = sbam_voffset(framed_header.size(), payload.size()); end[e] = sbam_voffset(framed_header.size(), payload.size() + pooled.record.size);
			payload.insert(payload.end(), records + pooled.at, records + pooled.at + pooled.record.size);
		}
		sorted_bam_frame(payload.data(), payload.size(), framed);
		row_file_bytes[row] = framed.size() - framed_before;
		uncompressed += payload.size(); blocks += sbam_block_count(payload.size());
	}
	SupportingWriter writer(prefix, framed_header.data(), framed_header.size(), n_rows, row_file_bytes.data());
	try {
		writer.push(framed.data(), framed.size());
		agpu_supporting_index_arrays arrays; memset(&arrays, 0, sizeof(arrays));
		arrays.n_rows = n_rows; arrays.n_records = n; arrays.row_first = row_first.data(); arrays.ref = ref.data(); arrays.pos = pos.data(); arrays.end_flag = end_flag.data(); arrays.bin = bin.data(); arrays.begin = begin.data(); arrays.end = end.data();
		writer.index(arrays, ref_length.data(), (uint32_t) ref_length.size());
		writer.commit();
	} catch (...) { writer.abandon(); throw; }
	if (info) { memset(info, 0, sizeof(*info)); info->rows = n_rows; info->records = n; info->uncompressed_bytes = uncompressed; info->file_bytes = framed.size(); info->blocks = blocks; info->windows = framed.empty() ? 0 : 1; info->window_bytes = framed.size(); }
}

}
