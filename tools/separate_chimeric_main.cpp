// tools/separate_chimeric_main.cpp -- the host side of -c, and pass C of the device's loop body stepped on the host, under a sanitizer (tools/sanitize_separate_chimeric.sh builds this file together with the host sources, ASan + UBSan
// linked in): the two passes of the host ingest over (C, R), then the same with C cut short at every byte of its last records -- a stream that ends inside a record must be
// refused ("failed to load alignments"), never read past its end, and one that ends between two records is a shorter file, not an error.
//   separate_chimeric_main assembly.fa annotation.gtf C.bam R.bam scratch_directory [records to cut: 3]
// Both passes of the device's loop body are stepped (replay_group_as with its role, name_is_taken over the names of pass C laid out as the device holds them, normalize_plan) and
// the union is compared with the batch of the host ingest, name by name with the number of alignments; R is stepped if it is an uncompressed BAM stream, too.
// C.bam must be an uncompressed BAM stream (tools/split_chimeric.py writes stored BGZF; `python tools/bam_to_sam.py` or zcat give the stream).  Exit code 0 if every ingest did
// what it should; the sanitizers abort on their own findings.
#include "../include/arriba_host.h"
#include "../arriba_amd/csrc/device/ingest_core.hpp" // the loop body of the kernels, stepped here on the host (its functions are host and device code)
#include <cstdio>
#include <algorithm>
#include <map>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static std::vector<unsigned char> read_file(const char* path) {
	std::vector<unsigned char> bytes;
	FILE* file = fopen(path, "rb");
	if (!file) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
	unsigned char buffer[1 << 16];
	size_t got;
	while ((got = fread(buffer, 1, sizeof(buffer), file)) > 0) bytes.insert(bytes.end(), buffer, buffer + got);
	fclose(file);
	return bytes;
}

int main(int argc, char** argv) {
	if (argc != 6 && argc != 7) { fprintf(stderr, "usage: separate_chimeric_main assembly.fa annotation.gtf C.bam R.bam scratch_directory [records to cut: 3]\n"); return 2; }
	const size_t cut_records = argc == 7 ? (size_t) atoi(argv[6]) : 3;
	ahost_session* session = ahost_open(argv[1], argv[2], NULL, NULL, NULL);
	if (!session) { fprintf(stderr, "%s\n", ahost_last_error()); return 2; }
	uint64_t fragments = 0, malformed = 0;
	if (ahost_ingest_separate(session, argv[3], argv[4], 0, 100, &fragments, &malformed) != 0) { fprintf(stderr, "whole files: %s\n", ahost_last_error()); return 1; }
	const uint64_t whole = ahost_batch_view(session)->n;
	printf("whole files: %llu fragments behind the separate chimeric file (%llu malformed), %llu behind the main alignments\n", (unsigned long long) fragments, (unsigned long long) malformed, (unsigned long long) whole);
	const std::vector<unsigned char> stream = read_file(argv[3]);
	if (stream.size() < 12 || memcmp(stream.data(), "BAM\1", 4) != 0) { fprintf(stderr, "%s is not an uncompressed BAM stream\n", argv[3]); return 2; }
	// the record chain: where every record starts
	auto word = [&stream](size_t at) { return (size_t) stream[at] | (size_t) stream[at + 1] << 8 | (size_t) stream[at + 2] << 16 | (size_t) stream[at + 3] << 24; };
	size_t at = 8 + word(4);
	const size_t n_ref = word(at);
	at += 4;
	for (size_t r = 0; r < n_ref; ++r) at += 8 + word(at);
	std::vector<size_t> starts;
	while (at + 4 <= stream.size()) { starts.push_back(at); at += 4 + word(at); }
	if (at != stream.size() || starts.size() < 4) { fprintf(stderr, "%s: the records do not end where the file ends, or there are fewer than four\n", argv[3]); return 2; }
	{ // pass C of the device code stepped over the same bytes: replay_group_as<ROLE_SEPARATE_CHIMERIC> and the sanity check per read name, in the order of the stream -- the
	  // fragments and the malformed count must be those of the host ingest; and the key of a QNAME taken from a packed name must be the key of the record (the look-up of pass R)
		std::vector<uint64_t> offsets(starts.begin(), starts.end());
		std::vector<uint32_t> identity(n_ref);
		for (size_t r = 0; r < n_ref; ++r) identity[r] = (uint32_t) r;
		std::vector<uint8_t> bits(offsets.size(), agpu::RECORD_ACTIVE);
		agpu::IngestContext context;
		memset(&context, 0, sizeof(context));
		context.stream.bytes = stream.data(); context.stream.size = stream.size(); context.stream.record_offset = offsets.data(); context.stream.n_records = offsets.size();
		context.stream.n_targets = (uint32_t) n_ref; context.stream.tid_to_contig = identity.data(); context.stream.hit_index = nullptr;
		context.record_bits = bits.data(); context.max_itd_length = 100;
		std::map<std::string, std::vector<uint32_t> > groups;
		for (uint32_t r = 0; r < offsets.size(); ++r) {
			const agpu::Rec record = agpu::load_record(context.stream, r);
			const uint32_t length = agpu::qname_length(record);
			if (agpu::name_key(record, 1, 0) != agpu::qname_bytes_key(record.name, length)) { fprintf(stderr, "record %u: qname_bytes_key is not name_key(record, 1, 0)\n", r); return 1; }
			groups[std::string((const char*) record.name, length)].push_back(r);
		}
		uint64_t stepped_fragments = 0, stepped_malformed = 0;
		std::map<std::string, uint32_t> stepped; // name -> alignments, of the fragments both passes leave
		std::vector<std::string> survivors;     // of pass C: what pass R finds taken
		auto no_viral_count = [](uint32_t) {};
		for (std::map<std::string, std::vector<uint32_t> >::const_iterator group = groups.begin(); group != groups.end(); ++group) {
			agpu::FragmentPlan plain; agpu::TandemPlan itd; agpu::GroupTally tally = { 0, 0, 0 };
			agpu::replay_group_as<agpu::ROLE_SEPARATE_CHIMERIC>(context, group->second.data(), (uint32_t) group->second.size(), plain, itd, tally, no_viral_count, nullptr, 0, 0, agpu::TakenNames());
			stepped_malformed += tally.malformed;
			if (plain.count == 0) continue;
			agpu::Fragment3 fragment;
			if (agpu::normalize_plan(context.stream, plain, nullptr, fragment)) {
				++stepped_fragments;
				survivors.push_back(group->first + ",1");
				if (!fragment.single_end) stepped[group->first + ",1"] = fragment.n; // (a single-end fragment does not pass the second sanity check)
			} else ++stepped_malformed;
		}
		if (stepped_fragments != fragments || stepped_malformed != malformed) {
			fprintf(stderr, "pass C stepped with the device code: %llu fragments, %llu malformed; the host ingest: %llu, %llu\n", (unsigned long long) stepped_fragments, (unsigned long long) stepped_malformed, (unsigned long long) fragments, (unsigned long long) malformed);
			return 1;
		}
		printf("pass C stepped with the device code: %llu fragments, %llu malformed, as the host ingest\n", (unsigned long long) stepped_fragments, (unsigned long long) stepped_malformed);

		// pass R stepped the same way over the bytes of R (an uncompressed BAM stream whose references stand in the order of the session's contigs): the names pass C left as the
		// device holds them -- packed names, their offsets, the sorted keys with their rows -- looked up by name_is_taken, replay_group_as<ROLE_SEPARATE_RNA>, the sanity check;
		// then both passes as one in name order against the batch of the host ingest: every name and its number of alignments
		std::string pool; std::vector<uint64_t> name_offset(1, 0);
		for (size_t k = 0; k < survivors.size(); ++k) { pool += survivors[k]; name_offset.push_back(pool.size()); }
		std::vector<std::pair<uint64_t, uint32_t> > keyed;
		for (size_t k = 0; k < survivors.size(); ++k) keyed.push_back(std::make_pair(agpu::qname_bytes_key((const uint8_t*) survivors[k].data(), (uint32_t) survivors[k].size() - 2), (uint32_t) k));
		std::sort(keyed.begin(), keyed.end());
		std::vector<uint64_t> taken_keys; std::vector<uint32_t> taken_rows;
		for (size_t k = 0; k < keyed.size(); ++k) { taken_keys.push_back(keyed[k].first); taken_rows.push_back(keyed[k].second); }
		agpu::TakenNames taken = { taken_keys.data(), taken_rows.data(), (uint64_t) taken_keys.size(), pool.data(), name_offset.data() };
		const std::vector<unsigned char> rna = read_file(argv[4]);
		if (rna.size() >= 12 && memcmp(rna.data(), "BAM\1", 4) == 0) {
			auto rna_word = [&rna](size_t at) { return (size_t) rna[at] | (size_t) rna[at + 1] << 8 | (size_t) rna[at + 2] << 16 | (size_t) rna[at + 3] << 24; };
			size_t rna_at = 8 + rna_word(4);
			const size_t rna_refs = rna_word(rna_at);
			rna_at += 4;
			for (size_t r = 0; r < rna_refs; ++r) rna_at += 8 + rna_word(rna_at);
			std::vector<uint64_t> rna_offsets;
			while (rna_at + 4 <= rna.size()) { rna_offsets.push_back(rna_at); rna_at += 4 + rna_word(rna_at); }
			const agpu_annotation_view* annotation = ahost_annotation_view(session);
			const agpu_genome_view* genome = ahost_genome_view(session);
			std::vector<uint32_t> rna_identity(rna_refs);
			for (size_t r = 0; r < rna_refs; ++r) rna_identity[r] = (uint32_t) r;
			std::vector<uint8_t> rna_bits(rna_offsets.size(), agpu::RECORD_SKIPPED);
			agpu::IngestContext second;
			memset(&second, 0, sizeof(second));
			second.stream.bytes = rna.data(); second.stream.size = rna.size(); second.stream.record_offset = rna_offsets.data(); second.stream.n_records = rna_offsets.size();
			second.stream.n_targets = (uint32_t) rna_refs; second.stream.tid_to_contig = rna_identity.data();
			second.record_bits = rna_bits.data(); second.max_itd_length = 100;
			second.genome.n_contigs = genome->n_contigs; second.genome.contig_offset = genome->contig_offset; second.genome.contig_bits = genome->contig_bits; second.genome.bases = genome->bases;
			agpu::AnnotationView& a = second.annotation;
			a.n_genes = annotation->n_genes; a.gene_contig = annotation->gene_contig; a.gene_start = annotation->gene_start; a.gene_end = annotation->gene_end; a.gene_bits = annotation->gene_bits;
			a.gene_exonic_length = annotation->gene_exonic_length;
			a.gene_index.n_contigs = annotation->gene_index.n_contigs; a.gene_index.contig_offset = annotation->gene_index.contig_offset; a.gene_index.keys = annotation->gene_index.keys;
			a.gene_index.member_offset = annotation->gene_index.member_offset; a.gene_index.members = annotation->gene_index.members;
			std::map<std::string, std::vector<uint32_t> > rna_groups;
			for (uint32_t r = 0; r < rna_offsets.size(); ++r) { // (what record_parse_kernel<ROLE_SEPARATE_RNA> decides)
				const agpu::Rec record = agpu::load_record(second.stream, r);
				if ((record.flag & agpu::BAMF_UNMAP) || ((record.flag & agpu::BAMF_PAIRED) && (record.flag & agpu::BAMF_MUNMAP))) continue;
				rna_bits[r] = agpu::RECORD_ACTIVE | (agpu::scan_aux(record.aux, record.end).has_sa ? agpu::RECORD_HAS_SA : 0);
				rna_groups[std::string((const char*) record.name, agpu::qname_length(record))].push_back(r);
			}
			for (std::map<std::string, std::vector<uint32_t> >::const_iterator group = rna_groups.begin(); group != rna_groups.end(); ++group) {
				agpu::FragmentPlan plain; agpu::TandemPlan itd; agpu::GroupTally tally = { 0, 0, 0 };
				agpu::replay_group_as<agpu::ROLE_SEPARATE_RNA>(second, group->second.data(), (uint32_t) group->second.size(), plain, itd, tally, no_viral_count, nullptr, 0, 0, taken);
				agpu::Fragment3 fragment;
				if (plain.count > 0 && agpu::normalize_plan(second.stream, plain, nullptr, fragment)) {
					if (stepped.count(group->first + ",1")) { fprintf(stderr, "%s,1: inserted by pass R although pass C holds it\n", group->first.c_str()); return 1; }
					stepped[group->first + ",1"] = fragment.n;
				}
				if (itd.plan.count > 0 && agpu::normalize_plan(second.stream, itd.plan, &itd.tandem, fragment)) stepped[group->first + ",1ITD"] = fragment.n;
			}
			const agpu_batch_view* batch = ahost_batch_view(session);
			if (stepped.size() != batch->n) { fprintf(stderr, "both passes stepped with the device code: %zu fragments; the host ingest: %llu\n", stepped.size(), (unsigned long long) batch->n); return 1; }
			uint64_t row = 0;
			for (std::map<std::string, uint32_t>::const_iterator fragment = stepped.begin(); fragment != stepped.end(); ++fragment, ++row) {
				uint32_t length = 0;
				const char* name = ahost_fragment_name(session, row, &length);
				if (std::string(name, length) != fragment->first || batch->n_aln[row] != fragment->second) {
					fprintf(stderr, "fragment %llu: stepped %s with %u alignments, the host ingest %.*s with %u\n", (unsigned long long) row, fragment->first.c_str(), fragment->second, (int) length, name, (unsigned int) batch->n_aln[row]);
					return 1;
				}
			}
			printf("both passes stepped with the device code: %zu fragments, names and alignment counts as the host ingest\n", stepped.size());
		} else printf("R is no uncompressed BAM stream: pass R was not stepped\n");
	}
	{ // two names under one key: the key is forced (no seed reaches the look-up), the bytes decide
		const std::string pool = "ABCD,1WXYZ,1";
		const uint64_t name_offset[3] = { 0, 6, 12 }, keys[2] = { agpu::qname_bytes_key((const uint8_t*) "WXYZ", 4), agpu::qname_bytes_key((const uint8_t*) "WXYZ", 4) };
		const uint32_t rows[2] = { 0, 1 };
		const agpu::TakenNames forced = { keys, rows, 2, pool.data(), name_offset };
		const agpu::TakenNames only_other = { keys, rows, 1, pool.data(), name_offset }; // the key of WXYZ, the bytes of ABCD
		if (!agpu::name_is_taken(forced, (const uint8_t*) "WXYZ", 4) || agpu::name_is_taken(only_other, (const uint8_t*) "WXYZ", 4) || agpu::name_is_taken(forced, (const uint8_t*) "WXY", 3)) {
			fprintf(stderr, "name_is_taken: a key hit must be confirmed on the bytes of the name\n");
			return 1;
		}
		printf("two names with one key do not block each other\n");
	}
	if (cut_records == 0 || cut_records > starts.size()) { ahost_close(session); return 0; }
	const size_t first_cut = starts[starts.size() - cut_records]; // the last records, byte by byte
	const std::string cut_path = std::string(argv[5]) + "/cut.bam";
	unsigned int refused = 0, accepted = 0;
	for (size_t size = first_cut; size < stream.size(); ++size) {
		FILE* file = fopen(cut_path.c_str(), "wb");
		if (!file || fwrite(stream.data(), 1, size, file) != size) { fprintf(stderr, "cannot write %s\n", cut_path.c_str()); return 2; }
		fclose(file);
		bool between_records = false;
		for (size_t k = starts.size() - cut_records; k < starts.size(); ++k) between_records = between_records || starts[k] == size;
		const int status = ahost_ingest_separate(session, cut_path.c_str(), argv[4], 0, 100, &fragments, &malformed);
		if (between_records) {
			if (status != 0) { fprintf(stderr, "cut at %zu (between two records): refused: %s\n", size, ahost_last_error()); return 1; }
			++accepted;
		} else {
			if (status == 0) { fprintf(stderr, "cut at %zu (inside a record): accepted\n", size); return 1; }
			if (strstr(ahost_last_error(), "failed to load alignments") == NULL) { fprintf(stderr, "cut at %zu: refused with another message: %s\n", size, ahost_last_error()); return 1; }
			++refused;
		}
	}
	remove(cut_path.c_str());
	printf("the separate chimeric file cut short: %u cuts inside a record refused, %u cuts between records accepted\n", refused, accepted);
	ahost_close(session);
	return 0;
}
