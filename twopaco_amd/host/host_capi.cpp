// host_capi.cpp -- plain-C entry points over the C++ host layer, for language bindings (the
// Python tests and bench.py reach CreateEnumerator, the text packer and the seed tables through
// these with ctypes).  Not part of the device ABI (include/twopaco_hip.h).
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "filterplan.h"
#include "graphformat.h"
#include "seed.h"
#include "streamfastaparser.h"
#include "textpack.h"
#include "vertexenumerator.h"

namespace
{
	thread_local std::string g_error;
	char * Dup(const std::string & s)
	{
		char * p = new char[s.size() + 1];
		std::memcpy(p, s.c_str(), s.size() + 1);
		return p;
	}

	// What every tpch_create_enumerator* shares: the file names, the options every one sets, the log stream and what becomes of it,
	// and the call.  `fill` sets the option fields of its entry point and throws its refusal.  outFile NULL: as empty.
	template<class Fill>
	void * Create(const char ** files, int nfiles, uint64_t k, uint64_t filterBits, uint64_t q, uint64_t rounds, uint64_t threads, uint64_t abundance,
		const char * tmpDir, const char * outFile, int pinned, uint64_t seed, int device, char ** log, Fill fill)
	{
		std::stringstream ss;
		try
		{
			std::vector<std::string> names(files, files + nfiles);
			TwoPaCo::EnumeratorOptions opt;
			opt.pinnedSeed = pinned != 0;
			opt.seed = seed;
			opt.device = device;
			fill(opt);
			std::unique_ptr<TwoPaCo::VertexEnumerator> e = TwoPaCo::CreateEnumerator(names, k, filterBits, q, rounds, threads, abundance, tmpDir, outFile ? outFile : "", ss, opt);
			if (log) *log = Dup(ss.str());
			return e.release();
		}
		catch (std::exception & e)
		{
			g_error = e.what();
			if (log) *log = Dup(ss.str());
			return 0;
		}
	}

	void SetGraph(TwoPaCo::EnumeratorOptions & opt, const char * graphFormat, const char * graphFile, int graphPrefix, int graphThreads)
	{
		opt.graphFormat = graphFormat ? graphFormat : "";
		opt.graphFile = graphFile ? graphFile : "";
		opt.graphPrefix = graphPrefix != 0;
		opt.graphThreads = size_t(graphThreads < 1 ? 1 : graphThreads);
	}

	namespace GF = TwoPaCo::GraphFormat;

	void SetLinks(TwoPaCo::EnumeratorOptions & opt, const char * linksFile, int graphCompact)
	{
		GF::SetTable(opt.tables, GF::LINKS, 0, linksFile, 0);
		opt.graphCompact = graphCompact != 0;
	}
}

extern "C"
{
	const char * tpch_last_error() { return g_error.c_str(); }
	void tpch_free(void * p) { delete[] static_cast<char*>(p); }

	// q x 5 seed table for `--seed seed` (pinned != 0) or from /dev/urandom
	int tpch_seed_table(uint64_t seed, int pinned, int q, int bits, uint64_t * table)
	{
		try
		{
			std::vector<uint64_t> t = TwoPaCo::MakeSeedTable(size_t(q), size_t(bits), pinned != 0, seed);
			std::memcpy(table, t.data(), t.size() * sizeof(uint64_t));
			return 0;
		}
		catch (std::exception & e) { g_error = e.what(); return -1; }
	}

	// ---- `-f auto` (filterplan.h): the count behind 16384 HyperLogLog registers (tpc_distinct_sketch), and the filter size and
	// rounds for a count.  No device.  out[5] = L, rounds, clipped, L_fp, L_mem; *falseMarks = predicted false marks per position.
	double tpch_hll_estimate(const uint8_t * registers, uint64_t m) { return TwoPaCo::HllEstimate(registers, size_t(m)); }
	int tpch_filter_plan(uint64_t distinctEdges, int q, uint64_t textLength, uint64_t filterBytesCap, int userRounds, int * out, double * falseMarks)
	{
		if (q < 1 || userRounds < 0 || !out) { g_error = "tpch_filter_plan: bad arguments"; return -1; }
		const TwoPaCo::FilterPlan plan = TwoPaCo::PlanFilter(distinctEdges, unsigned(q), textLength, filterBytesCap, unsigned(userRounds));
		out[0] = int(plan.filterBits); out[1] = int(plan.rounds); out[2] = plan.clipped ? 1 : 0; out[3] = int(plan.bitsForTarget); out[4] = int(plan.bitsForMemory);
		if (falseMarks) *falseMarks = plan.falseMarks;
		return 0;
	}

	// ---- packed text handle -------------------------------------------------------------
	void * tpch_text_new() { TwoPaCo::PackedText * t = new TwoPaCo::PackedText(); t->BeginText(); return t; }
	void tpch_text_free(void * h) { delete static_cast<TwoPaCo::PackedText*>(h); }
	int tpch_text_add_fasta(void * h, const char ** files, int nfiles, int threads)
	{
		try
		{
			TwoPaCo::PackedText * t = static_cast<TwoPaCo::PackedText*>(h);
			std::vector<std::string> names(files, files + nfiles);
			TwoPaCo::PackedText fresh;
			TwoPaCo::PackFastaFiles(names, size_t(threads), fresh);
			*t = fresh;
			return 0;
		}
		catch (std::exception & e) { g_error = e.what(); return -1; }
	}

	// one record given as codes 0..3, 4 = N
	void tpch_text_add_codes(void * h, const uint8_t * codes, uint64_t n)
	{
		TwoPaCo::PackedText * t = static_cast<TwoPaCo::PackedText*>(h);
		t->AppendCodes(codes, n);
		t->EndRecord(n);
	}

	uint64_t tpch_text_length(void * h) { return static_cast<TwoPaCo::PackedText*>(h)->length; }
	uint64_t tpch_text_words(void * h) { return static_cast<TwoPaCo::PackedText*>(h)->bases.size(); }
	const uint64_t * tpch_text_bases(void * h) { return static_cast<TwoPaCo::PackedText*>(h)->bases.data(); }
	const uint32_t * tpch_text_nmask(void * h) { return static_cast<TwoPaCo::PackedText*>(h)->nmask.data(); }
	uint32_t tpch_text_records(void * h) { return uint32_t(static_cast<TwoPaCo::PackedText*>(h)->recStart.size()); }
	const uint64_t * tpch_text_rec_start(void * h) { return static_cast<TwoPaCo::PackedText*>(h)->recStart.data(); }
	const uint64_t * tpch_text_rec_length(void * h) { return static_cast<TwoPaCo::PackedText*>(h)->recLength.data(); }

	// ---- CreateEnumerator ------------------------------------------------------------------
	// Returns an enumerator handle (or NULL; message via tpch_last_error); *log receives the
	// logStream text (free with tpch_free).
	void * tpch_create_enumerator(const char ** files, int nfiles, uint64_t k, uint64_t filterBits, uint64_t q, uint64_t rounds,
		uint64_t threads, uint64_t abundance, const char * tmpDir, const char * outFile, int pinned, uint64_t seed, int device,
		int testFirst, char ** log)
	{
		return Create(files, nfiles, k, filterBits, q, rounds, threads, abundance, tmpDir, outFile, pinned, seed, device, log, [&](TwoPaCo::EnumeratorOptions & opt)
		{
			opt.insertTestFirst = testFirst != 0;
		});
	}

	// the same with EnumeratorOptions::autoFilterSize (`-f auto`): the filter size comes from the device's sketch of the distinct
	// edges; rounds = 0 lets the plan choose them too.  graphFormat may be NULL or empty (no graph)
	void * tpch_create_enumerator_auto(const char ** files, int nfiles, uint64_t k, uint64_t q, uint64_t rounds,
		uint64_t threads, uint64_t abundance, const char * tmpDir, const char * outFile, int pinned, uint64_t seed, int device,
		const char * graphFormat, const char * graphFile, char ** log)
	{
		return Create(files, nfiles, k, 0, q, rounds == 0 ? 1 : rounds, threads, abundance, tmpDir, outFile, pinned, seed, device, log, [&](TwoPaCo::EnumeratorOptions & opt)
		{
			opt.autoFilterSize = true;
			opt.autoRounds = rounds == 0;
			opt.graphFormat = graphFormat ? graphFormat : "";
			opt.graphFile = graphFile ? graphFile : "";
		});
	}

	// the same with the multi-GPU knobs: gpus ranks, transport (rccl != 0: RCCL), emulate != 0: all ranks on `device`,
	// forceSharded != 0: the sharded path even for one GPU
	void * tpch_create_enumerator_mgpu(const char ** files, int nfiles, uint64_t k, uint64_t filterBits, uint64_t q, uint64_t rounds,
		uint64_t threads, uint64_t abundance, const char * tmpDir, const char * outFile, int pinned, uint64_t seed, int device,
		int gpus, int rccl, int emulate, int forceSharded, char ** log)
	{
		return Create(files, nfiles, k, filterBits, q, rounds, threads, abundance, tmpDir, outFile, pinned, seed, device, log, [&](TwoPaCo::EnumeratorOptions & opt)
		{
			opt.gpus = gpus;
			opt.rccl = rccl != 0;
			opt.emulateRanks = emulate != 0;
			opt.forceSharded = forceSharded != 0;
		});
	}

	// the same as tpch_create_enumerator with --graph (EnumeratorOptions::graphFormat ...): graphFormat gfa1 | gfa2 | fasta into
	// graphFile; outFile may be empty, then the junction stream is not written
	void * tpch_create_enumerator_graph(const char ** files, int nfiles, uint64_t k, uint64_t filterBits, uint64_t q, uint64_t rounds,
		uint64_t threads, uint64_t abundance, const char * tmpDir, const char * outFile, int pinned, uint64_t seed, int device,
		int testFirst, const char * graphFormat, const char * graphFile, int graphPrefix, int graphThreads, char ** log)
	{
		return Create(files, nfiles, k, filterBits, q, rounds, threads, abundance, tmpDir, outFile, pinned, seed, device, log, [&](TwoPaCo::EnumeratorOptions & opt)
		{
			opt.insertTestFirst = testFirst != 0;
			SetGraph(opt, graphFormat, graphFile, graphPrefix, graphThreads);
			if (opt.graphFormat.empty()) throw std::runtime_error("The graph format must be one of gfa1, gfa2, fasta");
		});
	}

	// the same as tpch_create_enumerator with --colors (EnumeratorOptions::tables): colorsBy file | sequence into colorsFile;
	// graphFormat may be NULL or empty (no graph); outFile may be empty, then the junction stream is not written
	void * tpch_create_enumerator_colors(const char ** files, int nfiles, uint64_t k, uint64_t filterBits, uint64_t q, uint64_t rounds,
		uint64_t threads, uint64_t abundance, const char * tmpDir, const char * outFile, int pinned, uint64_t seed, int device,
		int testFirst, const char * graphFormat, const char * graphFile, int graphPrefix, int graphThreads, const char * colorsBy, const char * colorsFile, char ** log)
	{
		return Create(files, nfiles, k, filterBits, q, rounds, threads, abundance, tmpDir, outFile, pinned, seed, device, log, [&](TwoPaCo::EnumeratorOptions & opt)
		{
			opt.insertTestFirst = testFirst != 0;
			SetGraph(opt, graphFormat, graphFile, graphPrefix, graphThreads);
			GF::SetTable(opt.tables, GF::COLORS, colorsBy, colorsFile, 0);
			if (!opt.tables.On(GF::COLORS)) throw std::runtime_error("The colours must be one of file, sequence");
		});
	}

	// the same as tpch_create_enumerator_colors with --links / --graph-compact (EnumeratorOptions::tables, graphCompact): linksFile
	// NULL or empty: no link table; colorsBy NULL or empty: no colour table
	void * tpch_create_enumerator_links(const char ** files, int nfiles, uint64_t k, uint64_t filterBits, uint64_t q, uint64_t rounds,
		uint64_t threads, uint64_t abundance, const char * tmpDir, const char * outFile, int pinned, uint64_t seed, int device,
		int testFirst, const char * graphFormat, const char * graphFile, int graphPrefix, int graphThreads, const char * colorsBy, const char * colorsFile,
		const char * linksFile, int graphCompact, char ** log)
	{
		return Create(files, nfiles, k, filterBits, q, rounds, threads, abundance, tmpDir, outFile, pinned, seed, device, log, [&](TwoPaCo::EnumeratorOptions & opt)
		{
			opt.insertTestFirst = testFirst != 0;
			SetGraph(opt, graphFormat, graphFile, graphPrefix, graphThreads);
			GF::SetTable(opt.tables, GF::COLORS, colorsBy, colorsFile, 0);
			SetLinks(opt, linksFile, graphCompact);
			if (!opt.tables.On(GF::LINKS) && !opt.graphCompact) throw std::runtime_error("One of the link table's file and the compact graph is required");
		});
	}

	// the same as tpch_create_enumerator_links with --distances (EnumeratorOptions::tables):
	// distancesBy file | sequence into distancesFile, phylipFile NULL or empty: no PHYLIP matrix; linksFile NULL or empty: no link
	// table; colorsBy NULL or empty: no colour table; autoFilter != 0: `-f auto` (EnumeratorOptions::autoFilterSize, filterBits is
	// ignored and rounds = 0 lets the plan choose them too, as tpch_create_enumerator_auto)
	void * tpch_create_enumerator_distances(const char ** files, int nfiles, uint64_t k, uint64_t filterBits, uint64_t q, uint64_t rounds,
		uint64_t threads, uint64_t abundance, const char * tmpDir, const char * outFile, int pinned, uint64_t seed, int device,
		int testFirst, const char * graphFormat, const char * graphFile, int graphPrefix, int graphThreads, const char * colorsBy, const char * colorsFile,
		const char * linksFile, int graphCompact, const char * distancesBy, const char * distancesFile, const char * phylipFile, int autoFilter, char ** log)
	{
		return Create(files, nfiles, k, autoFilter ? 0 : filterBits, q, autoFilter && rounds == 0 ? 1 : rounds, threads, abundance, tmpDir, outFile, pinned, seed, device, log,
			[&](TwoPaCo::EnumeratorOptions & opt)
		{
			opt.insertTestFirst = testFirst != 0;
			SetGraph(opt, graphFormat, graphFile, graphPrefix, graphThreads);
			GF::SetTable(opt.tables, GF::COLORS, colorsBy, colorsFile, 0);
			SetLinks(opt, linksFile, graphCompact);
			if (!distancesBy || !*distancesBy || !distancesFile || !*distancesFile) throw std::runtime_error("The distance table needs its colours, one of file, sequence, and a file name");
			GF::SetTable(opt.tables, GF::DISTANCES, distancesBy, distancesFile, phylipFile);
			opt.autoFilterSize = autoFilter != 0;
			opt.autoRounds = autoFilter != 0 && rounds == 0;
		});
	}

	// the same as tpch_create_enumerator_distances with --components instead (EnumeratorOptions::tables): componentsBy file | sequence into componentsFile, membersFile NULL or empty: no members file
	void * tpch_create_enumerator_components(const char ** files, int nfiles, uint64_t k, uint64_t filterBits, uint64_t q, uint64_t rounds,
		uint64_t threads, uint64_t abundance, const char * tmpDir, const char * outFile, int pinned, uint64_t seed, int device,
		int testFirst, const char * graphFormat, const char * graphFile, int graphPrefix, int graphThreads, const char * colorsBy, const char * colorsFile,
		const char * linksFile, int graphCompact, const char * componentsBy, const char * componentsFile, const char * membersFile, char ** log)
	{
		return Create(files, nfiles, k, filterBits, q, rounds, threads, abundance, tmpDir, outFile, pinned, seed, device, log, [&](TwoPaCo::EnumeratorOptions & opt)
		{
			opt.insertTestFirst = testFirst != 0;
			SetGraph(opt, graphFormat, graphFile, graphPrefix, graphThreads);
			GF::SetTable(opt.tables, GF::COLORS, colorsBy, colorsFile, 0);
			SetLinks(opt, linksFile, graphCompact);
			if (!componentsBy || !*componentsBy || !componentsFile || !*componentsFile) throw std::runtime_error("The component table needs its colours, one of file, sequence, and a file name");
			GF::SetTable(opt.tables, GF::COMPONENTS, componentsBy, componentsFile, membersFile);
		});
	}

	// The text of the compacted graph from an EVENT TABLE (include/twopaco_hip.h: name / first bits / begin / end per event,
	// seq_event_begin[0 .. n_seq] per sequence) and the FASTA files, into out_path: graphformat.h without any device.  format
	// gfa1 | gfa2 | fasta, prefix = graphdump's --prefix.  0, or nonzero with tpch_last_error.
	int tpch_graph_format(const char ** files, int nfiles, uint64_t k, const char * format, int prefix, int threads, uint64_t n_events,
		const int64_t * name, const uint32_t * first_words, const uint32_t * begin, const uint32_t * end, uint64_t n_seq,
		const uint32_t * seq_event_begin, const char * out_path)
	{
		try
		{
			namespace GF = TwoPaCo::GraphFormat;
			const std::string fmt = format ? format : "";
			if (!GF::IsGraphFormat(fmt)) throw std::runtime_error("The graph format must be one of gfa1, gfa2, fasta");
			if (!out_path || !*out_path) throw std::runtime_error("The graph needs an output file name");
			if (nfiles < 0 || (nfiles && !files)) throw std::runtime_error("FASTA file names required");
			const size_t workers = size_t(threads < 1 ? 1 : (threads > 16 ? 16 : threads));
			std::vector<std::string> names(files, files + nfiles);
			GF::InputSequences seq;
			GF::LoadedSequences loaded;
			GF::LoadSequences(names, fmt == "fasta" ? true : prefix != 0, workers, seq, loaded);
			GF::EventTable table;
			table.events = n_events;
			table.name = name; table.first = first_words; table.begin = begin; table.end = end;
			table.sequences = n_seq;
			table.seqEventBegin = seq_event_begin;
			GF::CheckEventTable(table, loaded, size_t(k), workers);
			GF::WriteGraphFile(table, seq, loaded, size_t(k), fmt, workers, out_path);
			return 0;
		}
		catch (std::exception & e) { g_error = e.what(); return -1; }
	}

	void tpch_enumerator_free(void * h) { delete static_cast<TwoPaCo::VertexEnumerator*>(h); }
	uint64_t tpch_vertices_count(void * h) { return static_cast<TwoPaCo::VertexEnumerator*>(h)->GetVerticesCount(); }
	int64_t tpch_get_id(void * h, const char * kmer) { return static_cast<TwoPaCo::VertexEnumerator*>(h)->GetId(kmer); }
	int tpch_hash_seed(void * h, uint64_t * table)
	{
		const TwoPaCo::VertexRollingHashSeed & s = static_cast<TwoPaCo::VertexEnumerator*>(h)->GetHashSeed();
		std::memcpy(table, s.Table().data(), s.Table().size() * sizeof(uint64_t));
		return int(s.HashFunctionsNumber());
	}
}
