// junctiondump.cpp -- the `graphdump` tool: converts de_bruijn.bin (junctionapi.h) to text formats.
//
// Downstream consumer of the junction stream, kept flag- and byte-compatible with the reference's
// graphdump (reference src/graphdump/graphdump.cpp) so that pipelines built on it are unchanged:
//   graphdump <infile> -f seq|group|dot|gfa1|gfa2|fasta -k <k> [-s <fasta>]... [--prefix] [--gpu [<device>]] [--threads <n>] [--text host|device]
//             [--compact]  |  --colors file|sequence [--colors-out <path>]  |  --links [--links-out <path>]
//             |  --bubbles file|sequence [--bubbles-out <path>]
//             |  --distances file|sequence [--distances-out <path>] [--distances-phylip <path>]
//             |  --components file|sequence [--components-out <path>] [--components-members <path>]
//             |  --superbubbles file|sequence [--superbubbles-out <path>] [--superbubbles-members <path>] [--superbubbles-max <n>]
//             |  --anchors file|sequence [--anchors-ref <colour>] [--anchors-out <path>] [--anchors-paf <path>]
//             |  --locate file|sequence --locate-in <q.fa> [--locate-in ...] [--locate-out <path>] [--locate-walks <path>]
//             (the last seven instead of -f)
// Formats (reference line numbers):
//   seq    "chr pos id" per junction occurrence, file order (:160-168)
//   group  occurrences of the same junction id on one line, lines ordered by their first position (:122-158)
//   dot    two arcs per pair of consecutive junctions of a sequence (:588-609)
//   gfa1 / gfa2 / fasta  the compacted graph: one segment per pair of consecutive junctions; its id packs the
//          smaller-id end junction, its strand and the following character (:44-113), or a fresh id from
//          2^34 upwards when that character is 'N'; segments are printed on first sight, then the occurrence
//          (C / F line), the link to the previous segment of the sequence (L / E) and one path per sequence
//          (P / O) (:379-480, :504-585).
// Differences from the reference that do not change the output: the "seen" set is a hash set instead of a
// 2^35-bit vector (4 GiB), and output is buffered.  Where the reference reads out of bounds (a .bin whose first
// sequences were too short to be dispatched, so that sequence ids and FASTA records get out of step) it prints
// garbage before its "The input is corrupted"; this tool reports the error without the garbage.
// --gpu (an addition; without it nothing changes): for gfa1 / gfa2 / fasta the serial part of the walk -- segment names,
// fresh names of 'N' segments, first sight -- is computed on the device (csrc/tpc_segments.hip through the tpc_segments_*
// group of include/twopaco_hip.h, loaded with dlopen: the binary has no link-time dependency on the device library), after
// which every output line depends only on its own event and the one before it, and `--threads` workers format contiguous
// chunks of events that go to stdout in order (graphformat.h, shared with `twopaco --graph`; its input is the event table the
// device leaves -- name, first sight, the two positions of every event, the events of every sequence -- fetched with
// tpc_segments_fetch_*).  No device or no library with --gpu is an error: there is no fallback.
// --text device (with --gpu; the default is host): the text itself is rendered on the device from the table that is already
// there (csrc/tpc_segtext.hip: tpc_segments_text_plan / _text_write) and this process only writes it -- the table is not
// fetched and --threads formats nothing.  The bytes are the same.  The table is complete before the first byte is printed, so
// a stream the walk refuses prints its error and nothing else (the host paths have printed the header lines by then).
// --colors file|sequence [--colors-out <path>] (an addition; instead of -f): the segment colour table -- for every segment of the
// graph (the body-carrying S lines of gfa1, in their order) its length, its occurrences (the C lines), how many of them are
// forward, and which colours hold it, a colour being an input file or an input sequence; then the histogram of segments by
// their number of colours -- as TSV (graphformat.h: WriteColors).  Without --gpu the serial walk collects the event table and
// ComputeColors groups it; with --gpu the device does both (csrc/tpc_colors.hip); the bytes are the same.  A stream the walk
// refuses prints the walk's error and nothing else, and creates no file.
// --links [--links-out <path>] (an addition; instead of -f): the link table -- every distinct link between two segments once, as it
// is spelled where the walk first meets it, with the number of its occurrences (the L lines of gfa1) and how many of them are
// spelled that way; (a, b) and (-b, -a) are one link -- as TSV (graphformat.h: WriteLinks; include/twopaco_hip.h defines the table).
// Without --gpu the serial walk collects the event table and ComputeLinks groups it; with --gpu the device does both
// (csrc/tpc_links.hip); the bytes are the same.
// -f gfa1 --compact (an addition): the gfa1 text without the per-sequence S header lines, without the C lines, and with every link
// once (the L line of its first occurrence); the H line, the S lines with a body and the P lines are byte for byte those of gfa1.
// Serial or with --gpu, the same bytes.  The whole table is known before the first byte is printed: a stream the walk refuses
// prints the walk's error and nothing else.
// --bubbles file|sequence [--bubbles-out <path>] (an addition; instead of -f): the simple bubbles of the graph -- where two segments
// leave one side of a segment, touch nothing else and meet again at one side of another; include/twopaco_hip.h defines them -- as
// TSV with the colour rows of the two arms (graphformat.h: WriteBubbles).  Without --gpu the serial walk, then ComputeColors,
// ComputeLinks and ComputeBubbles; with --gpu the three device stages over one segment build (csrc/tpc_bubbles.hip); the bytes are
// the same.  Every byte waits until the table is complete: a stream the walk refuses prints the walk's error and nothing else.
// --distances file|sequence [--distances-out <path>] [--distances-phylip <path>] (an addition; instead of -f): how much every colour
// shares with every other one -- the segments and the edges ((k+1)-mers) two colours both hold; include/twopaco_hip.h defines them --
// as TSV of integers (graphformat.h: WriteDistances) and, asked for, as a PHYLIP square matrix of Jaccard distances over edges.
// Without --gpu the serial walk, then ComputeColors and ComputeDistances; with --gpu the colour stage and the distance stage over one
// segment build (csrc/tpc_distances.hip); the bytes are the same.  A stream the walk refuses prints the walk's error and nothing else.
// --components file|sequence [--components-out <path>] [--components-members <path>] (an addition; instead of -f): the connected
// components of the graph -- which segments hang together, a segment that no link touches being a component of one;
// include/twopaco_hip.h defines them -- as TSV of integers with every component's segments, links, bases, edges, occurrences and
// colours (graphformat.h: WriteComponents) and, asked for, the component of every segment (WriteComponentMembers).  Without --gpu the
// serial walk, then ComputeColors, ComputeLinks and ComputeComponents; with --gpu the colour stage, the link stage and the component
// stage over one segment build (csrc/tpc_components.hip); the bytes are the same.  Beside --colors, --bubbles or --distances of the
// same colours it is written after them.  A stream the walk refuses prints the walk's error and nothing else.
// --superbubbles file|sequence [--superbubbles-out <path>] [--superbubbles-members <path>] [--superbubbles-max <n>] (an addition;
// instead of -f): the superbubbles of the graph, bounded to n sides inside (2 .. 62, default 62) -- where the genomes differ beyond
// two alleles; include/twopaco_hip.h defines them -- as TSV of integers (graphformat.h: WriteSuperbubbles) and, asked for, the inside
// sides of every row (WriteSuperbubbleMembers).  Without --gpu the serial walk, then ComputeColors, ComputeLinks and
// ComputeSuperbubbles; with --gpu the colour stage, the link stage and the superbubble stage over one segment build
// (csrc/tpc_superbubbles.hip); the bytes are the same.  Beside --colors, --bubbles, --distances or --components of the same colours it
// is written after them.  Its refusals are those of --bubbles.
// --anchors file|sequence [--anchors-ref <colour>] [--anchors-out <path>] [--anchors-paf <path>] (an addition; instead of -f): the
// anchor blocks against the reference colour (default 0) -- where every other colour matches it uniquely, in which order and on
// which strand; include/twopaco_hip.h defines them -- as TSV (graphformat.h: WriteAnchors) and, asked for, as PAF
// (WriteAnchorsPaf).  Without --gpu the serial walk, then ComputeAnchors; with --gpu the anchor stage over the segment build
// (csrc/tpc_anchors.hip); the bytes are the same.  Beside --colors, --bubbles, --distances, --components or --superbubbles of the
// same colours it is written after them; not with --links.
// --locate file|sequence --locate-in <q.fa> [--locate-in ...] [--locate-out <path>] [--locate-walks <path>] (an addition; instead of
// -f): the records of the query files looked up in the graph, window by window -- is a sequence that was no input in the graph,
// where, and in which colours; include/twopaco_hip.h defines index, hit, run and sums -- as TSV (graphformat.h: WriteLocate) and,
// asked for, the runs as a walks file (WriteLocateWalks).  Without --gpu the serial walk, then BuildEdgeIndex and ComputeLocate;
// with --gpu the edge index over the segment build and the queries through it in batches of whole records of at most 2^28
// positions (csrc/tpc_locate.hip); the bytes are the same.  Beside the other tables of the same colours it is written last; not
// with -f, --links, --compact or --text.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include <dlfcn.h>
#include <unistd.h>

#include "../../include/twopaco_hip.h"
#include "devicegraph.h"
#include "dnachar.h"
#include "graphformat.h"
#include "junctionapi.h"
#include "streamfastaparser.h"
#include "textpack.h"

namespace
{
	using TwoPaCo::DnaChar;
	using TwoPaCo::JunctionPosition;

	using namespace TwoPaCo::GraphFormat;  // Out, the sinks, LoadSequences, the parallel formatter (graphformat.h)
	using namespace TwoPaCo::DeviceGraph;  // the tables built on the device and fetched (devicegraph.h)

	// ---------------------------------------------------------------------------------------- seq / group / dot
	void DumpSeq(const std::string & binFile, Out & out)
	{
		TwoPaCo::JunctionPositionReader reader(binFile);
		for (JunctionPosition j; reader.NextJunctionPosition(j);)
		{
			out << uint64_t(j.GetChr()) << ' ' << uint64_t(j.GetPos()) << ' ' << int64_t(j.GetId()) << '\n';
		}
	}

	void DumpGroups(const std::string & binFile, Out & out)
	{
		struct Occ { int64_t id; uint32_t chr, pos; };
		std::vector<Occ> all;
		TwoPaCo::JunctionPositionReader reader(binFile);
		for (JunctionPosition j; reader.NextJunctionPosition(j);)
		{
			all.push_back(Occ{j.GetId(), j.GetChr(), j.GetPos()});
		}

		// one group per signed id, members in (chr, pos) order; groups in the order of their first member
		std::sort(all.begin(), all.end(), [](const Occ & a, const Occ & b)
		{
			if (a.id != b.id) return a.id < b.id;
			return a.chr != b.chr ? a.chr < b.chr : a.pos < b.pos;
		});

		std::vector<std::pair<size_t, size_t> > group;
		for (size_t i = 0; i < all.size();)
		{
			size_t j = i;
			while (j < all.size() && all[j].id == all[i].id) ++j;
			group.push_back(std::make_pair(i, j));
			i = j;
		}

		std::stable_sort(group.begin(), group.end(), [&all](const std::pair<size_t, size_t> & a, const std::pair<size_t, size_t> & b)
		{
			const Occ & x = all[a.first];
			const Occ & y = all[b.first];
			return x.chr != y.chr ? x.chr < y.chr : x.pos < y.pos;
		});

		for (const std::pair<size_t, size_t> & g : group)
		{
			for (size_t i = g.first; i < g.second; i++) out << uint64_t(all[i].chr) << ' ' << uint64_t(all[i].pos) << "; ";
			out << '\n';
		}
	}

	void DumpDot(const std::string & binFile, Out & out)
	{
		out << "digraph G\n{\n\trankdir = LR\n";
		TwoPaCo::JunctionPositionReader reader(binFile);
		JunctionPosition prev;
		for (JunctionPosition now; reader.NextJunctionPosition(now); prev = now)
		{
			if (now.GetChr() != prev.GetChr()) continue;
			out << '\t' << int64_t(prev.GetId()) << " -> " << int64_t(now.GetId()) << "[color=\"blue\", label=\"chr=" << uint64_t(prev.GetChr()) << " pos="
				<< uint64_t(prev.GetPos()) << "\"]\n";
			out << '\t' << int64_t(-now.GetId()) << " -> " << int64_t(-prev.GetId()) << "[color=\"red\", label=\"chr=" << uint64_t(prev.GetChr()) << " pos="
				<< uint64_t(prev.GetPos()) << "\"]\n";
		}

		out << "}\n";
	}

	// ---------------------------------------------------------------------------------------- segments
	// Segment naming, reference graphdump.cpp:44-113.  The segment between junctions a (left) and b (right) is
	// oriented from its end with the smaller |id| (ties: forward unless both ids are 0); `next` is the character
	// that follows the start junction's k-mer in that orientation.  The name of a reverse segment is negative, except
	// between two ids of 0, where the reference keeps it positive.
	class SegmentNamer
	{
	public:
		SegmentNamer() : nextUnique_(int64_t(1) << 34) {}

		int64_t Name(int64_t leftId, int64_t rightId, char afterLeft, char beforeRightComplemented)
		{
			const int64_t LIMIT = int64_t(1) << 31;  // MAX_JUNCTION_ID
			// compared as they stand: the magnitude of INT64_MIN does not exist (the reference negates it all the same)
			if (leftId >= LIMIT || leftId <= -LIMIT || rightId >= LIMIT || rightId <= -LIMIT)
			{
				throw std::runtime_error("A vertex id is too large, cannot generate GFA");
			}

			const int64_t l = Magnitude(leftId), r = Magnitude(rightId);

			const bool forward = l < r || (l == r && l > 0);
			const char next = forward ? afterLeft : beforeRightComplemented;
			const int64_t start = forward ? leftId : -rightId;
			if (next == 'N')
			{
				return nextUnique_++;
			}

			int64_t name = static_cast<int64_t>(DnaChar::MakeUpChar(next));
			if (start < 0)
			{
				name |= 1 << 2;
				name |= Magnitude(start) << 3;
			}
			else
			{
				name |= start << 3;
			}

			// negated when the start is not the left junction as it stands (graphdump.cpp:88-91): every reverse segment but the one
			// between two ids of 0, whose start -0 is the left id
			return start != leftId ? -name : name;
		}

	private:
		int64_t nextUnique_;
	};

	void ListSequences(const std::vector<std::string> & fasta, bool prefixed, InputSequences & seq)
	{
		size_t index = 0;  // the reference never advances this counter: every prefix is "s0_" (graphdump.cpp:176-192)
		for (size_t fileNumber = 0; fileNumber < fasta.size(); fileNumber++)
		{
			const std::string & f = fasta[fileNumber];
			TwoPaCo::StreamFastaParser parser(f);
			while (parser.ReadRecord())
			{
				const std::string id = prefixed ? "s" + std::to_string(index) + "_" + parser.GetCurrentHeader() : parser.GetCurrentHeader();
				seq.name.push_back(id);
				seq.file[id] = f;
				seq.fileIndex.push_back(uint32_t(fileNumber));
				uint64_t n = 0;
				for (char ch; parser.GetChar(ch);) ++n;
				seq.length.push_back(n);
			}
		}
	}

	// one sequence after the other, across the files
	class SequenceCursor
	{
	public:
		explicit SequenceCursor(const std::vector<std::string> & fasta) : fasta_(fasta), file_(0), parser_(0)
		{
			if (!fasta_.empty()) parser_ = new TwoPaCo::StreamFastaParser(fasta_[0]);
		}

		~SequenceCursor() { delete parser_; }

		bool Next(std::string & body)
		{
			body.clear();
			while (file_ < fasta_.size())
			{
				if (parser_->ReadRecord())
				{
					for (char ch; parser_->GetChar(ch);) body.push_back(ch);
					return true;
				}

				delete parser_;
				parser_ = 0;
				if (++file_ < fasta_.size()) parser_ = new TwoPaCo::StreamFastaParser(fasta_[file_]);
			}

			return false;
		}

	private:
		SequenceCursor(const SequenceCursor &);
		void operator = (const SequenceCursor &);
		std::vector<std::string> fasta_;
		size_t file_;
		TwoPaCo::StreamFastaParser * parser_;
	};

	// The walk shared by gfa1 / gfa2 / fasta (reference graphdump.cpp:398-480).  Consecutive records of the same
	// sequence bound a segment; a change of sequence must step the sequence id by exactly one.
	void WalkSegments(const std::string & binFile, const std::vector<std::string> & fasta, size_t k, SegmentSink & sink)
	{
		SegmentNamer namer;
		std::unordered_set<int64_t> seen;
		SequenceCursor cursor(fasta);
		TwoPaCo::JunctionPositionReader reader(binFile);
		std::string chr;
		size_t sequence = 0;
		JunctionPosition left;
		if (!reader.NextJunctionPosition(left))
		{
			sink.EndOfSequence(sequence);
			return;
		}

		// The reference indexes sequence 0 with whatever the first record holds (out of bounds when the first
		// sequences are shorter than k and were skipped); here that input is reported as what it is.
		cursor.Next(chr);
		if (left.GetChr() != 0)
		{
			throw std::runtime_error("The input is corrupted");
		}

		for (JunctionPosition right; reader.NextJunctionPosition(right); left = right)
		{
			if (left.GetChr() != right.GetChr())
			{
				sink.EndOfSequence(sequence);
				cursor.Next(chr);
				if (right.GetChr() != ++sequence)
				{
					throw std::runtime_error("The input is corrupted");
				}

				continue;
			}

			if (right.GetPos() <= left.GetPos() || uint64_t(right.GetPos()) + k > chr.size())
			{
				throw std::runtime_error("The input is corrupted");
			}

			SegmentEvent e;
			e.id = namer.Name(left.GetId(), right.GetId(), chr[left.GetPos() + k], DnaChar::ReverseChar(chr[right.GetPos() - 1]));
			e.size = uint64_t(right.GetPos()) + k - left.GetPos();
			e.first = seen.insert(Magnitude(e.id)).second;
			e.begin = left.GetPos();
			e.end = right.GetPos();
			e.sequence = sequence;
			sink.Segment(e, chr, k);
		}

		sink.EndOfSequence(sequence);
	}

	// ---------------------------------------------------------------------------------------- --colors, serial
	// The event table of the stream, collected from the serial walk: what the device leaves after tpc_segments_build_*.
	class EventCollector : public SegmentSink
	{
	public:
		std::vector<int64_t> name;
		std::vector<uint32_t> first, begin, end, sequenceOf;

		void Segment(const SegmentEvent & e, const std::string &, size_t)
		{
			if ((name.size() & 31) == 0) first.push_back(0);
			if (e.first) first.back() |= uint32_t(1) << (name.size() & 31);
			name.push_back(e.id);
			begin.push_back(uint32_t(e.begin));
			end.push_back(uint32_t(e.end));
			sequenceOf.push_back(uint32_t(e.sequence));
		}

		void EndOfSequence(size_t) {}

		// seqEventBegin must outlive the table
		void Table(size_t sequences, std::vector<uint32_t> & seqEventBegin, EventTable & table) const
		{
			seqEventBegin.assign(sequences + 1, 0);
			for (uint32_t s : sequenceOf)
			{
				if (s >= sequences) throw std::runtime_error("The input is corrupted");
				seqEventBegin[s + 1] += 1;
			}

			for (size_t s = 0; s < sequences; s++) seqEventBegin[s + 1] += seqEventBegin[s];
			table.events = name.size();
			table.name = name.data();
			table.first = first.data();
			table.begin = begin.data();
			table.end = end.data();
			table.sequences = sequences;
			table.seqEventBegin = seqEventBegin.data();
		}
	};

	// --distances beside another table of the same colours: the file names of the distance table, written after that table from the
	// same walk (or segment build) and the same colour table
	struct DistancesWanted
	{
		bool on;
		std::string out, phylip;
		DistancesWanted() : on(false) {}
	};

	void DumpColors(const std::string & binFile, const std::vector<std::string> & fasta, size_t k, bool prefix, bool bySequence, const std::string & outPath,
		const DistancesWanted & also = DistancesWanted())
	{
		InputSequences seq;
		ListSequences(fasta, prefix, seq);
		EventCollector events;
		WalkSegments(binFile, fasta, k, events);
		std::vector<uint32_t> seqEventBegin;
		EventTable table;
		events.Table(seq.name.size(), seqEventBegin, table);
		ColorMap map;
		MakeColorMap(seq, fasta, bySequence, map);
		ColorTable colors;
		ComputeColors(table, k, map.colorOfSequence, map.label.size(), colors);
		DistanceTable distances;
		if (also.on) ComputeDistances(table, colors, distances);
		WriteColors(table, k, map, colors, outPath);
		if (also.on) WriteDistanceFiles(k, map, colors.Rows(), distances, also.out, also.phylip);
	}

	// ---------------------------------------------------------------------------------------- --links and --compact, serial
	struct SerialTable
	{
		InputSequences seq;
		LoadedSequences loaded;
		EventCollector events;
		std::vector<uint32_t> seqEventBegin;
		EventTable table;
		LinkTable links;
	};

	// the walk's event table and its links; nothing is printed before both are complete
	void WalkLinks(const std::string & binFile, const std::vector<std::string> & fasta, size_t k, bool prefix, bool bodies, SerialTable & out)
	{
		if (bodies) LoadSequences(fasta, prefix, 1, out.seq, out.loaded);
		else ListSequences(fasta, prefix, out.seq);
		WalkSegments(binFile, fasta, k, out.events);
		out.events.Table(out.seq.name.size(), out.seqEventBegin, out.table);
		ComputeLinks(out.table, out.links);
	}

	uint64_t CountFirstBits(const EventTable & table)
	{
		uint64_t n = 0;
		for (uint64_t w = 0; w < (table.events + 31) / 32; w++) n += uint64_t(__builtin_popcount(table.first[w]));
		return n;
	}

	void DumpLinks(const std::string & binFile, const std::vector<std::string> & fasta, size_t k, bool prefix, const std::string & outPath)
	{
		SerialTable t;
		WalkLinks(binFile, fasta, k, prefix, false, t);
		WriteLinks(t.table, k, CountFirstBits(t.table), t.links, outPath);
	}

	void DumpCompact(const std::string & binFile, const std::vector<std::string> & fasta, size_t k, bool prefix)
	{
		SerialTable t;
		WalkLinks(binFile, fasta, k, prefix, true, t);
		t.table.linkFirst = t.links.linkFirst.data();
		Out head(false);
		HeaderLines("gfa1", t.seq, head, true);
		std::fwrite(head.Text().data(), 1, head.Text().size(), stdout);
		FormatEvents(t.table, t.seq, t.loaded, k, "gfa1", 1, -1, 0);
	}

	// --bubbles, serial: the walk, then the three serial statements one after the other
	void DumpBubbles(const std::string & binFile, const std::vector<std::string> & fasta, size_t k, bool prefix, bool bySequence, const std::string & outPath,
		const DistancesWanted & also = DistancesWanted())
	{
		SerialTable t;
		WalkLinks(binFile, fasta, k, prefix, false, t);
		ColorMap map;
		MakeColorMap(t.seq, fasta, bySequence, map);
		ColorTable colors;
		ComputeColors(t.table, k, map.colorOfSequence, map.label.size(), colors);
		BubbleTable bubbles;
		ComputeBubbles(t.table, t.links, bubbles);
		DistanceTable distances;
		if (also.on) ComputeDistances(t.table, colors, distances);
		WriteBubbles(t.table, k, map, colors, t.links.Rows(), bubbles, outPath);
		if (also.on) WriteDistanceFiles(k, map, colors.Rows(), distances, also.out, also.phylip);
	}

	struct ArgError
	{
		std::string what, arg;
		ArgError(const std::string & w, const std::string & a) : what(w), arg(a) {}
	};

	// --anchors beside another table of the same colours, or alone: the reference colour and the file names (out empty: stdout)
	struct AnchorsWanted
	{
		bool on;
		uint32_t ref;
		std::string out, paf;
		AnchorsWanted() : on(false), ref(0) {}
	};

	// the reference colour must be one of the map's: known only once the input's files and sequences are
	void CheckAnchorsRef(const AnchorsWanted & anchors, const ColorMap & map)
	{
		if (anchors.on && anchors.ref >= map.label.size())
		{
			throw ArgError("Value '" + std::to_string(anchors.ref) + "' does not meet constraint: a colour index below " + std::to_string(map.label.size()), "Argument: (--anchors-ref)");
		}
	}

	// --locate beside another table of the same colours, or alone: the query files and the file names (out empty: stdout, walks empty: none)
	struct LocateWanted
	{
		bool on;
		std::vector<std::string> in;
		std::string out, walks;
		LocateWanted() : on(false) {}
	};

	// Positions of packed query text per device call, whole records: 2^28, or what TWOPACO_LOCATE_BATCH says (tests: a small query in
	// several batches)
	uint64_t LocateBatchPositions()
	{
		const char * e = std::getenv("TWOPACO_LOCATE_BATCH");
		const long long n = e && *e ? std::atoll(e) : 0;
		return n > 0 ? uint64_t(n) : uint64_t(1) << 28;
	}

	// --components beside another table of the same colours, or alone: the file names of the component table (out empty: stdout)
	struct ComponentsWanted
	{
		bool on;
		std::string out, members;
		ComponentsWanted() : on(false) {}
	};

	// --superbubbles beside another table of the same colours, or alone: the file names (out empty: stdout) and the bound
	struct SuperbubblesWanted
	{
		bool on;
		std::string out, members;
		uint32_t maxInside;
		SuperbubblesWanted() : on(false), maxInside(62) {}
	};

	// --components, --superbubbles and / or --anchors, serial, alone or beside --colors / --bubbles / --distances of the same colours: one
	// walk, the serial statements one after the other, then the tables in the order colours or bubbles, distances, components,
	// superbubbles, anchors
	void DumpComponents(const std::string & binFile, const std::vector<std::string> & fasta, size_t k, bool prefix, bool bySequence, const ComponentsWanted & want,
		bool colorsToo, bool bubblesToo, const std::string & firstOut, bool distancesToo, const DistancesWanted & distancesTo, const SuperbubblesWanted & super,
		const AnchorsWanted & anchorsTo = AnchorsWanted(), const LocateWanted & locateTo = LocateWanted())
	{
		SerialTable t;
		WalkLinks(binFile, fasta, k, prefix, locateTo.on, t);   // (the edge index reads the letters)
		ColorMap map;
		MakeColorMap(t.seq, fasta, bySequence, map);
		CheckAnchorsRef(anchorsTo, map);
		ColorTable colors;
		ComputeColors(t.table, k, map.colorOfSequence, map.label.size(), colors);
		BubbleTable bubbles;
		if (bubblesToo) ComputeBubbles(t.table, t.links, bubbles);
		DistanceTable distances;
		if (distancesToo) ComputeDistances(t.table, colors, distances);
		ComponentTable components;
		if (want.on) ComputeComponents(t.table, k, t.links, colors, components);
		SuperbubbleTable superbubbles;
		if (super.on) ComputeSuperbubbles(t.table, k, t.links, colors, super.maxInside, superbubbles);
		AnchorTable anchors;
		if (anchorsTo.on) ComputeAnchors(t.table, k, map.colorOfSequence, map.label.size(), anchorsTo.ref, anchors);
		InputSequences queries;
		LocateTable locate;
		if (locateTo.on)
		{
			LoadedSequences queryLetters;
			LoadSequences(locateTo.in, false, 1, queries, queryLetters);
			CheckEventTable(t.table, t.loaded, k, 1);
			EdgeIndex index;
			BuildEdgeIndex(t.table, t.loaded, k, index);
			ComputeLocate(index, colors, queryLetters, locate);
		}

		if (colorsToo) WriteColors(t.table, k, map, colors, firstOut);
		if (bubblesToo) WriteBubbles(t.table, k, map, colors, t.links.Rows(), bubbles, firstOut);
		if (distancesToo) WriteDistanceFiles(k, map, colors.Rows(), distances, distancesTo.out, distancesTo.phylip);
		if (want.on) WriteComponentFiles(t.table, k, map, colors, t.links.Rows(), components, want.out, want.members);
		if (super.on) WriteSuperbubbleFiles(t.table, k, map, colors, t.links.Rows(), superbubbles, super.out, super.members);
		if (anchorsTo.on) WriteAnchorFiles(t.table, k, map, t.seq, anchors, anchorsTo.out, anchorsTo.paf);
		if (locateTo.on) WriteLocateFiles(t.table, k, map, colors, queries, locate, locateTo.out, locateTo.walks);
	}

	// --distances, serial: the walk, the colour table, then the serial statement of the matrices
	void DumpDistances(const std::string & binFile, const std::vector<std::string> & fasta, size_t k, bool prefix, bool bySequence, const std::string & outPath,
		const std::string & phylipPath)
	{
		InputSequences seq;
		ListSequences(fasta, prefix, seq);
		EventCollector events;
		WalkSegments(binFile, fasta, k, events);
		std::vector<uint32_t> seqEventBegin;
		EventTable table;
		events.Table(seq.name.size(), seqEventBegin, table);
		ColorMap map;
		MakeColorMap(seq, fasta, bySequence, map);
		ColorTable colors;
		ComputeColors(table, k, map.colorOfSequence, map.label.size(), colors);
		DistanceTable distances;
		ComputeDistances(table, colors, distances);
		WriteDistanceFiles(k, map, colors.Rows(), distances, outPath, phylipPath);
	}

	// ---------------------------------------------------------------------------------------- --gpu
	double MsSince(const std::chrono::steady_clock::time_point & t0)
	{
		return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	}

	struct DumpStats
	{
		std::string path, text;
		uint64_t events, segments, nNamed, deviceBytes, streamBytes, textBytes, tableBytes;
		double loadMs, packMs, deviceMs, kernelMs, indexMs, formatMs, textKernelMs, colorsKernelMs, colorsMs, linksKernelMs, linksMs;
		uint64_t links, linkOccurrences, bubbles, components, largestComponent, superbubbles, superbubbleMembers, superbubblesUnmirrored, anchorBlocks, anchors;
		double bubblesKernelMs, bubblesMs, distancesKernelMs, distancesMs, componentsKernelMs, componentsMs, superbubblesKernelMs, superbubblesMs, anchorsKernelMs, anchorsMs;
		double edgesKernelMs, edgesMs, locateKernelMs, locateMs;
		uint64_t locateRuns, locateBatches;
		size_t threads;
		DumpStats() : path("host"), text("host"), events(0), segments(0), nNamed(0), deviceBytes(0), streamBytes(0), textBytes(0), tableBytes(0), loadMs(0), packMs(0),
			deviceMs(0), kernelMs(0), indexMs(0), formatMs(0), textKernelMs(0), colorsKernelMs(0), colorsMs(0), linksKernelMs(0), linksMs(0), links(0), linkOccurrences(0), bubbles(0), components(0), largestComponent(0), bubblesKernelMs(0), bubblesMs(0), distancesKernelMs(0), distancesMs(0),
			componentsKernelMs(0), componentsMs(0), superbubbles(0), superbubbleMembers(0), superbubblesUnmirrored(0), anchorBlocks(0), anchors(0), superbubblesKernelMs(0), superbubblesMs(0), anchorsKernelMs(0), anchorsMs(0), edgesKernelMs(0), edgesMs(0), locateKernelMs(0), locateMs(0), locateRuns(0), locateBatches(0), threads(1) {}

		// TWOPACO_GRAPHDUMP_STATS=<file>: one JSON object (never on stderr, whose bytes are compared with the reference's)
		void Write() const
		{
			const char * file = std::getenv("TWOPACO_GRAPHDUMP_STATS");
			if (!file || !*file) return;
			FILE * f = std::fopen(file, "w");
			if (!f) return;
			std::fprintf(f, "{\"path\": \"%s\", \"events\": %llu, \"segments\": %llu, \"n_named\": %llu, \"device_ms\": %.3f, \"kernel_ms\": %.3f, \"load_ms\": %.3f, "
				"\"pack_ms\": %.3f, \"index_ms\": %.3f, \"format_ms\": %.3f, \"threads\": %llu, \"device_bytes\": %llu, \"stream_bytes\": %llu, \"text_bytes\": %llu, "
				"\"table_bytes\": %llu, \"text\": \"%s\", \"text_kernel_ms\": %.3f, \"colors_kernel_ms\": %.3f, \"colors_ms\": %.3f, "
				"\"links_kernel_ms\": %.3f, \"links_ms\": %.3f, \"links\": %llu, \"link_occurrences\": %llu, "
				"\"bubbles_kernel_ms\": %.3f, \"bubbles_ms\": %.3f, \"bubbles\": %llu, \"distances_kernel_ms\": %.3f, \"distances_ms\": %.3f, "
				"\"components_kernel_ms\": %.3f, \"components_ms\": %.3f, \"components\": %llu, \"largest_component\": %llu, "
				"\"superbubbles_kernel_ms\": %.3f, \"superbubbles_ms\": %.3f, \"superbubbles\": %llu, \"superbubble_members\": %llu, \"superbubbles_unmirrored\": %llu, "
				"\"anchors_kernel_ms\": %.3f, \"anchors_ms\": %.3f, \"anchor_blocks\": %llu, \"anchors\": %llu, "
				"\"edges_kernel_ms\": %.3f, \"edges_ms\": %.3f, \"locate_kernel_ms\": %.3f, \"locate_ms\": %.3f, \"locate_runs\": %llu, \"locate_batches\": %llu}\n", path.c_str(), (unsigned long long)events, (unsigned long long)segments, (unsigned long long)nNamed, deviceMs, kernelMs, loadMs,
				packMs, indexMs, formatMs, (unsigned long long)threads, (unsigned long long)deviceBytes, (unsigned long long)streamBytes, (unsigned long long)textBytes,
				(unsigned long long)tableBytes, text.c_str(), textKernelMs, colorsKernelMs, colorsMs, linksKernelMs, linksMs, (unsigned long long)links,
				(unsigned long long)linkOccurrences, bubblesKernelMs, bubblesMs, (unsigned long long)bubbles, distancesKernelMs, distancesMs, componentsKernelMs, componentsMs,
				(unsigned long long)components, (unsigned long long)largestComponent, superbubblesKernelMs, superbubblesMs, (unsigned long long)superbubbles,
				(unsigned long long)superbubbleMembers, (unsigned long long)superbubblesUnmirrored, anchorsKernelMs, anchorsMs, (unsigned long long)anchorBlocks,
				(unsigned long long)anchors, edgesKernelMs, edgesMs, locateKernelMs, locateMs, (unsigned long long)locateRuns, (unsigned long long)locateBatches);
			std::fclose(f);
		}
	};

	// libtwopaco_hip.so, loaded when --gpu is given: ../lib beside the directory of the executable.  The entry points are those of
	// devicegraph.h, each found with dlsym.
	class DeviceLibrary : public TwoPaCo::DeviceGraph::Api
	{
	public:
		explicit DeviceLibrary(int device) : handle_(0)
		{
			char exe[4096];
			const ssize_t n = ::readlink("/proc/self/exe", exe, sizeof(exe) - 1);
			std::string dir = n > 0 ? std::string(exe, size_t(n)) : std::string();
			dir = dir.find('/') == std::string::npos ? std::string(".") : dir.substr(0, dir.rfind('/'));
			const std::string path = dir + "/../lib/libtwopaco_hip.so";
			handle_ = ::dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
			if (!handle_)
			{
				const char * why = ::dlerror();
				throw std::runtime_error("--gpu: cannot load " + path + (why ? std::string(": ") + why : std::string()));
			}

			Load([this](const char * name)
			{
				void * fn = ::dlsym(handle_, name);
				if (!fn) throw std::runtime_error(std::string("--gpu: libtwopaco_hip.so lacks ") + name);
				return fn;
			});

			check = [this](int rc, const char * what)
			{
				if (rc != 0) throw std::runtime_error(std::string("--gpu: tpc_") + what + " failed: " + last_error(ctx));
			};

			const int rc = ctx_create(device, &ctx);
			if (rc != 0 || !ctx)
			{
				ctx = 0;
				throw std::runtime_error("--gpu: no HIP device " + std::to_string(device) + " (tpc_ctx_create returned " + std::to_string(rc) + "); there is no CPU fallback behind --gpu");
			}
		}

		~DeviceLibrary()
		{
			if (ctx) ctx_destroy(ctx);
		}

	private:
		DeviceLibrary(const DeviceLibrary &);
		void operator = (const DeviceLibrary &);

		void * handle_;
	};

	// The front half of every device path: the stream's bytes and the packed text go up, the device builds the event table of
	// the stream (name, first sight, the two positions of every event, the events of every sequence).  counts: tpc_segments_counts;
	// sequences: how many the text holds; t0: when the device stage began.  Throws what the serial walk throws at a stream it refuses.
	void BuildTableOnDevice(DeviceLibrary & lib, const std::string & binFile, const std::vector<std::string> & fasta, size_t k, size_t threads,
		const LoadedSequences & loaded, DumpStats & stats, uint64_t * counts, size_t & sequences, std::chrono::steady_clock::time_point & t0)
	{
		const size_t SLOT_BYTES = 12;
		// the stream's bytes
		std::vector<char> bin;
		{
			std::ifstream in(binFile.c_str(), std::ios::binary);
			if (!in) throw std::runtime_error("Can't read the input file");
			in.seekg(0, std::ios::end);
			const std::streamoff size = in.tellg();
			in.seekg(0, std::ios::beg);
			if (size > 0)
			{
				bin.resize(size_t(size));
				in.read(&bin[0], size);
				bin.resize(size_t(in.gcount()));
			}
		}

		// the packed text and where the namer must not read 'N'
		t0 = std::chrono::steady_clock::now();
		TwoPaCo::PackedText text;
		TwoPaCo::PackFastaFiles(fasta, threads, text);
		if (text.recStart.size() != loaded.body.size()) throw std::runtime_error("--gpu: the packer and the parser disagree about the input sequences");
		std::vector<uint64_t> ambiguous;
		for (size_t r = 0; r < loaded.body.size(); r++)
		{
			if (text.recLength[r] != loaded.body[r].size()) throw std::runtime_error("--gpu: the packer and the parser disagree about the input sequences");
			for (uint64_t at : loaded.ambiguous[r]) ambiguous.push_back(text.recStart[r] + at);
		}

		stats.packMs = MsSince(t0);

		// the device stage
		t0 = std::chrono::steady_clock::now();
		lib.check(lib.seq_upload(lib.ctx, text.bases.data(), text.nmask.data(), text.length), "seq_upload");
		lib.check(lib.segments_build_host(lib.ctx, bin.data(), bin.size(), int(k), text.recStart.data(), text.recLength.data(), uint32_t(text.recStart.size()),
			ambiguous.data(), ambiguous.size()), "segments_build_host");
		std::vector<char>().swap(bin);
		uint64_t errorSlot = 0;
		int errorKind = 0;
		sequences = text.recStart.size();
		lib.check(lib.segments_counts(lib.ctx, counts), "segments_counts");
		lib.check(lib.segments_error(lib.ctx, &errorSlot, &errorKind), "segments_error");
		stats.path = "device";
		stats.events = counts[0];
		stats.segments = counts[1];
		stats.nNamed = counts[2];
		stats.tableBytes = counts[3];
		stats.deviceBytes = counts[5];
		stats.streamBytes = counts[4] * SLOT_BYTES;
		stats.textBytes = ((text.length + 31) / 32) * 12;
		stats.kernelMs = lib.kernel_ms(lib.ctx, TPC_K_SEGMENTS);
		if (errorKind != TPC_SEG_OK)
		{
			stats.deviceMs = MsSince(t0);
			stats.Write();
			// what the serial walk throws at this pair
			throw std::runtime_error(errorKind == TPC_SEG_ID_TOO_LARGE ? "A vertex id is too large, cannot generate GFA" : "The input is corrupted");
		}
	}

	// The event table of the last build, fetched whole.  Returns the milliseconds of the second half: the positions and the sequences'
	// ranges (DumpStats::indexMs)
	double FetchTable(DeviceLibrary & lib, Events & held)
	{
		FetchNames(lib, held);
		FetchFirst(lib, held);
		const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
		FetchPositions(lib, held);
		FetchSequences(lib, held);
		if (held.seqEventBegin[held.table.sequences] != held.table.events) throw std::runtime_error("--gpu: the device counted another number of segments than the stream holds");
		return MsSince(t0);
	}

	void TimingLine(const char * what, double ms, double kernelMs)
	{
		if (std::getenv("TWOPACO_TIMING")) std::fprintf(stderr, "[timing] %s on device: %.3f ms (kernels %.3f ms)\n", what, ms, kernelMs);
	}

	// The link table of the table on the device (csrc/tpc_links.hip), fetched: the rows, the first bits, or the number of rows alone.
	void LinksOnDevice(DeviceLibrary & lib, uint64_t events, bool rows, bool bits, LinkTable & links, DumpStats & stats)
	{
		const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
		BuildLinks(lib);
		stats.linksKernelMs = lib.kernel_ms(lib.ctx, TPC_K_LINKS);
		stats.links = FetchLinks(lib, events, rows, bits, links);
		stats.linkOccurrences = links.occurrences;
		stats.linksMs = MsSince(t0);
		TimingLine("link table", stats.linksMs, stats.linksKernelMs);
	}

	// What a --gpu run instead of -f writes: one of the colour, link and bubble tables into `out`, and / or the distance table and the
	// component table (alone, or beside the colour or the bubble table of the same colours, written after it).
	struct TablesWanted
	{
		bool colors, links, bubbles, distances, components, superbubbles, bySequence;
		std::string out, distancesOut, distancesPhylip, componentsOut, componentsMembers, superbubblesOut, superbubblesMembers;
		uint32_t superbubblesMax;
		AnchorsWanted anchors;
		LocateWanted locate;
	};

	// --colors, --links, --bubbles, --distances with --gpu: one segment build, the table stays on the device, and the stages that are
	// wanted run there in this order: colours (csrc/tpc_colors.hip), distances over their presence bits (csrc/tpc_distances.hip), links
	// (csrc/tpc_links.hip), bubbles over the link rows (csrc/tpc_bubbles.hip), components over the link rows and the colour rows
	// (csrc/tpc_components.hip).  Fetched is what the files print and no more: the event
	// table for the names and lengths of any rows; --distances alone fetches the two matrices, neither colour rows nor event table.
	void DumpTablesOnDevice(DeviceLibrary & lib, const std::string & binFile, const std::vector<std::string> & fasta, size_t k, size_t threads,
		const InputSequences & seq, const LoadedSequences & loaded, const TablesWanted & want, DumpStats & stats)
	{
		uint64_t counts[6] = {0, 0, 0, 0, 0, 0};
		size_t sequences = 0;
		std::chrono::steady_clock::time_point t0;
		BuildTableOnDevice(lib, binFile, fasta, k, threads, loaded, stats, counts, sequences, t0);
		ColorMap map;
		ColorTable colors;
		const bool colorTable = want.colors || want.bubbles || want.distances || want.components || want.superbubbles || want.locate.on;
		if (colorTable || want.anchors.on)
		{
			MakeColorMap(seq, fasta, want.bySequence, map);
			if (map.colorOfSequence.size() != sequences) throw std::runtime_error("--gpu: the packer and the parser disagree about the input sequences");
			CheckAnchorsRef(want.anchors, map);
		}

		if (colorTable)
		{
			const std::chrono::steady_clock::time_point c0 = std::chrono::steady_clock::now();
			BuildColors(lib, map);
			stats.colorsKernelMs = lib.kernel_ms(lib.ctx, TPC_K_COLORS);
			if (want.colors || want.bubbles || want.components || want.superbubbles || want.locate.on) FetchColors(lib, map, counts[1], colors);
			stats.colorsMs = MsSince(c0);
		}

		DistanceTable distances;
		if (want.distances)
		{
			const std::chrono::steady_clock::time_point d0 = std::chrono::steady_clock::now();
			BuildDistances(lib);
			stats.distancesKernelMs = lib.kernel_ms(lib.ctx, TPC_K_DISTANCES);
			if (!FetchDistances(lib, map.label.size(), counts[1], distances)) throw std::runtime_error("--gpu: the distance stage and the colour map disagree about the colours or the segments");
			stats.distancesMs = MsSince(d0);
			TimingLine("distance matrices", stats.distancesMs, stats.distancesKernelMs);
		}

		LinkTable links;
		if (want.links || want.bubbles || want.components || want.superbubbles) LinksOnDevice(lib, counts[0], want.links || want.bubbles, false, links, stats);
		BubbleTable bubbles;
		if (want.bubbles)
		{
			const std::chrono::steady_clock::time_point b0 = std::chrono::steady_clock::now();
			BuildBubbles(lib);
			stats.bubblesKernelMs = lib.kernel_ms(lib.ctx, TPC_K_BUBBLES);
			FetchBubbles(lib, bubbles);
			stats.bubbles = bubbles.source.size();
			stats.bubblesMs = MsSince(b0);
			TimingLine("bubble table", stats.bubblesMs, stats.bubblesKernelMs);
		}

		ComponentTable components;
		if (want.components)
		{
			const std::chrono::steady_clock::time_point p0 = std::chrono::steady_clock::now();
			BuildComponents(lib);
			stats.componentsKernelMs = lib.kernel_ms(lib.ctx, TPC_K_COMPONENTS);
			if (!FetchComponents(lib, counts[1], colors.Words(), components)) throw std::runtime_error("--gpu: the component stage and the segment table disagree about the segments");
			stats.components = components.Rows();
			stats.largestComponent = components.Largest();
			stats.componentsMs = MsSince(p0);
			TimingLine("component table", stats.componentsMs, stats.componentsKernelMs);
		}

		SuperbubbleTable superbubbles;
		if (want.superbubbles)
		{
			const std::chrono::steady_clock::time_point p0 = std::chrono::steady_clock::now();
			BuildSuperbubbles(lib, want.superbubblesMax);
			stats.superbubblesKernelMs = lib.kernel_ms(lib.ctx, TPC_K_SUPERBUBBLES);
			if (!FetchSuperbubbles(lib, counts[1], colors.Words(), superbubbles)) throw std::runtime_error("--gpu: the superbubble stage and the segment table disagree about the segments");
			stats.superbubbles = superbubbles.Rows();
			stats.superbubbleMembers = superbubbles.members.size();
			stats.superbubblesUnmirrored = superbubbles.unmirrored;
			stats.superbubblesMs = MsSince(p0);
			TimingLine("superbubble table", stats.superbubblesMs, stats.superbubblesKernelMs);
		}

		AnchorTable anchors;
		if (want.anchors.on)
		{
			// over the event table alone (csrc/tpc_anchors.hip): neither the colour rows nor the link rows are read
			const std::chrono::steady_clock::time_point a0 = std::chrono::steady_clock::now();
			BuildAnchors(lib, map, want.anchors.ref);
			stats.anchorsKernelMs = lib.kernel_ms(lib.ctx, TPC_K_ANCHORS);
			if (!FetchAnchors(lib, map, counts[0], counts[1], anchors)) throw std::runtime_error("--gpu: the anchor stage and the colour map disagree about the colours");
			stats.anchorBlocks = anchors.Rows();
			stats.anchors = anchors.Anchors();
			stats.anchorsMs = MsSince(a0);
			TimingLine("anchor table", stats.anchorsMs, stats.anchorsKernelMs);
		}

		InputSequences queries;
		LocateTable locate;
		if (want.locate.on)
		{
			// the edge index over the table and the text where they are, the colour rows of the build above (csrc/tpc_locate.hip)
			const std::chrono::steady_clock::time_point l0 = std::chrono::steady_clock::now();
			LoadedSequences queryLetters;
			LoadSequences(want.locate.in, false, threads, queries, queryLetters);
			uint64_t edges[6] = {0, 0, 0, 0, 0, 0};
			BuildEdges(lib, edges);
			stats.edgesKernelMs = lib.kernel_ms(lib.ctx, TPC_K_LOCATE);
			stats.edgesMs = MsSince(l0);
			TimingLine("edge index", stats.edgesMs, stats.edgesKernelMs);
			const std::chrono::steady_clock::time_point l1 = std::chrono::steady_clock::now();
			stats.locateBatches = LocateOnDevice(lib, edges, map.label.size(), counts[1], queryLetters, LocateBatchPositions(), locate, stats.locateKernelMs);
			stats.locateRuns = locate.Runs();
			stats.locateMs = MsSince(l1);
			TimingLine("locate", stats.locateMs, stats.locateKernelMs);
		}

		Events held(counts[0], sequences);
		if (want.colors || want.links || want.bubbles || want.components || want.superbubbles || want.anchors.on || want.locate.on) FetchTable(lib, held);
		stats.deviceMs = MsSince(t0);
		t0 = std::chrono::steady_clock::now();
		if (want.colors) WriteColors(held.table, k, map, colors, want.out);
		if (want.links) WriteLinks(held.table, k, counts[1], links, want.out);
		if (want.bubbles) WriteBubbles(held.table, k, map, colors, links.Rows(), bubbles, want.out);
		if (want.distances) WriteDistanceFiles(k, map, counts[1], distances, want.distancesOut, want.distancesPhylip);
		if (want.components) WriteComponentFiles(held.table, k, map, colors, stats.links, components, want.componentsOut, want.componentsMembers);
		if (want.superbubbles) WriteSuperbubbleFiles(held.table, k, map, colors, stats.links, superbubbles, want.superbubblesOut, want.superbubblesMembers);
		if (want.anchors.on) WriteAnchorFiles(held.table, k, map, seq, anchors, want.anchors.out, want.anchors.paf);
		if (want.locate.on) WriteLocateFiles(held.table, k, map, colors, queries, locate, want.locate.out, want.locate.walks);
		stats.formatMs = MsSince(t0);
		if (want.colors) TimingLine("colour table", stats.colorsMs, stats.colorsKernelMs);
	}

	// The device path of gfa1 / gfa2 / fasta.  `out` holds what main printed so far (the header lines).  The formatter of
	// graphformat.h reads the table and the letters, never the stream's bytes.
	void DumpSegmentsOnDevice(DeviceLibrary & lib, const std::string & binFile, const std::vector<std::string> & fasta, size_t k, size_t threads,
		const std::string & format, const InputSequences & seq, const LoadedSequences & loaded, Out & out, DumpStats & stats, bool textOnDevice, bool compact)
	{
		uint64_t counts[6] = {0, 0, 0, 0, 0, 0};
		size_t sequences = 0;
		std::chrono::steady_clock::time_point t0;
		BuildTableOnDevice(lib, binFile, fasta, k, threads, loaded, stats, counts, sequences, t0);
		if (textOnDevice)
		{
			// the text from the table where it is: nothing is fetched but the bytes to print
			TwoPaCo::GraphFormat::DeviceTextInput input;
			TwoPaCo::GraphFormat::MakeDeviceTextInput(seq, loaded, input);
			uint64_t total = 0, written = 0;
			lib.check(lib.segments_text_plan(lib.ctx, TwoPaCo::GraphFormat::DeviceTextFormat(format), input.names.data(), input.nameOffset.data(),
				input.ambiguousLetter.empty() ? 0 : input.ambiguousLetter.data(), &total), "segments_text_plan");
			uint64_t after[6] = {0, 0, 0, 0, 0, 0};
			lib.check(lib.segments_counts(lib.ctx, after), "segments_counts");
			stats.deviceBytes = after[5];
			stats.deviceMs = MsSince(t0);
			t0 = std::chrono::steady_clock::now();
			std::fwrite(out.Text().data(), 1, out.Text().size(), stdout);  // the header lines, held back until here
			out.Text().clear();
			std::fflush(stdout);
			// a regular file is written at its offset (pwrite), anything else in order
			const off_t at = ::lseek(STDOUT_FILENO, 0, SEEK_CUR);
			lib.check(lib.segments_text_write(lib.ctx, STDOUT_FILENO, at >= 0 ? uint64_t(at) : 0, 0, &written), "segments_text_write");
			if (written != total) throw std::runtime_error("--gpu: the text was not written in full");
			if (at >= 0) (void)::lseek(STDOUT_FILENO, at + off_t(written), SEEK_SET);
			stats.formatMs = MsSince(t0);
			stats.textKernelMs = lib.kernel_ms(lib.ctx, TPC_K_SEGTEXT);
			if (std::getenv("TWOPACO_TIMING")) std::fprintf(stderr, "[timing] graph text on device: %.3f ms\n", stats.formatMs);
			return;
		}

		// name and first sight, then where every event sits in the stream: its two positions and the events of every sequence, as
		// the device's scans left them
		Events held(counts[0], sequences);
		stats.indexMs = FetchTable(lib, held);
		EventTable & table = held.table;
		LinkTable links;
		if (compact)
		{
			LinksOnDevice(lib, counts[0], false, true, links, stats);
			table.linkFirst = links.linkFirst.data();
		}

		stats.deviceMs = MsSince(t0) - stats.indexMs;

		// format: contiguous chunks of events, each into its own buffer, buffers to stdout in order
		t0 = std::chrono::steady_clock::now();
		out.Flush();
		if (!out.Text().empty())
		{
			// (--compact holds its header line back until the table is known to be good)
			std::fwrite(out.Text().data(), 1, out.Text().size(), stdout);
			out.Text().clear();
		}

		FormatEvents(table, seq, loaded, k, format, threads, -1, 0);
		stats.formatMs = MsSince(t0);
	}

	// ---------------------------------------------------------------------------------------- command line
	void Usage()
	{
		std::printf("\nUSAGE: \n\n   graphdump  [-k <integer>] [-s <string>] ... -f <seq|group|dot|gfa1|gfa2|fasta> [--prefix] [--gpu [<device>]] [--threads <integer>] [--text <host|device>] [--colors <file|sequence>] [--colors-out <file name>] [--links] [--links-out <file name>] [--compact] [--bubbles <file|sequence>] [--bubbles-out <file name>] [--distances <file|sequence>] [--distances-out <file name>] [--distances-phylip <file name>] [--components <file|sequence>] [--components-out <file name>] [--components-members <file name>] [--superbubbles <file|sequence>] [--superbubbles-out <file name>] [--superbubbles-members <file name>] [--superbubbles-max <integer>] [--anchors <file|sequence>] [--anchors-ref <integer>] [--anchors-out <file name>] [--anchors-paf <file name>] [--] [--version] [-h] <file name>\n\n"
			"Where: \n\n"
			"   -k <integer>,  --kvalue <integer>\n     (required)  Value of k\n\n"
			"   -s <string>,  --seqfile <string>  (accepted multiple times)\n     sequences file name\n\n"
			"   -f <seq|group|dot|gfa1|gfa2|fasta>,  --format <seq|group|dot|gfa1|gfa2|fasta>\n     (required)  Output format\n\n"
			"   --prefix\n     Add a prefix to segments in GFA (in case if you have genomes with identical FASTA headers)\n\n"
			"   --gpu [<device>]\n     gfa1, gfa2, fasta: name and deduplicate the segments on HIP device <device> (default 0) and format the output with\n"
			"     several threads; the output is the same.  An error when there is no device: no CPU fallback.\n"
			"     (twopaco --graph <gfa1|gfa2|fasta> writes the same text from the process that enumerates the junctions.)\n\n"
			"   --threads <integer>\n     threads of --gpu (1..16, default 16)\n\n"
			"   --text <host|device>\n     with --gpu: host (default) formats the text with the threads above, device renders the same bytes on the\n"
			"     GPU and this process only writes them\n\n"
			"   --colors <file|sequence>\n     instead of -f: the segment colour table as TSV -- per segment of the graph its length, occurrences, forward\n"
			"     occurrences, number of colours and presence bits, a colour being an input file or an input sequence, then the\n"
			"     histogram of segments by number of colours.  Needs -k and -s.  With --gpu the table is grouped on the device.\n"
			"     Not with --text; --prefix is accepted and changes nothing (sequence names are not printed).\n\n"
			"   --colors-out <file name>\n     with --colors: write the table there instead of to the standard output\n\n"
			"   --links\n     instead of -f: the link table as TSV -- every distinct link between two segments once, as spelled where it is\n"
			"     first met (segment, strand, segment, strand), its occurrences (the L lines of gfa1) and how many of them are spelled\n"
			"     that way; a b and -b -a are one link.  Needs -k and -s.  With --gpu the links are found on the device.\n"
			"     Not with --colors or --text.\n\n"
			"   --links-out <file name>\n     with --links: write the table there instead of to the standard output\n\n"
			"   --compact\n     with -f gfa1: no per-sequence S header lines, no C lines, and every link once (the L line of its first\n"
			"     occurrence); everything else as gfa1.  Serial or with --gpu; not with --text device.\n\n"
			"   --bubbles <file|sequence>\n     instead of -f: the simple bubbles of the graph as TSV -- the places where two segments (the arms) leave one side of\n"
			"     a segment, touch nothing else and meet again at one side of another: a substitution or a short insertion or\n"
			"     deletion between genomes.  Per bubble its source, two arms and sink (segment, strand), then of the arms the lengths,\n"
			"     occurrences, numbers of colours and presence bits of --colors, and the number of colours that hold both arms;\n"
			"     in front the colours and the number of sides (oriented segments) by degree, 0 being the dead ends.  Simple bubbles\n"
			"     only: three alleles at one place, nested bubbles and superbubbles are not reported.  Needs -k and -s.  With --gpu\n"
			"     the bubbles are found on the device.  Not with --colors, --links, --compact or --text.\n\n"
			"   --bubbles-out <file name>\n     with --bubbles: write the table there instead of to the standard output\n\n"
			"   --distances <file|sequence>\n     instead of -f: how much every colour (file or sequence, as --colors) shares with every other one, as TSV of\n"
			"     integers: per colour its own segments and edges ((k+1)-mers), then for every pair i < j the segments and the edges\n"
			"     both hold.  Edges, not bases: neighbouring segments overlap by k bases.  Jaccard = e_ij / (e_ii + e_jj - e_ij).\n"
			"     Needs -k and -s.  With --gpu the matrices are summed on the device.  Goes with --colors or --bubbles of the\n"
			"     same colours (one walk and one colour table for both; that table is written first, this one after it); not with --links, --compact or --text.\n\n"
			"   --distances-out <file name>\n     with --distances: write the table there instead of to the standard output\n\n"
			"   --distances-phylip <file name>\n     with --distances: also write the Jaccard distances over edges as a relaxed PHYLIP square matrix there\n\n"
			"   --components <file|sequence>\n     instead of -f: the connected components of the graph as TSV of integers -- which segments hang together, a segment\n"
			"     that no link touches being a component of one.  Per component, numbered in the order gfa1 first prints a segment of\n"
			"     each: the name of its first segment, its segments, links, bases, edges ((k+1)-mers), occurrences, number of colours\n"
			"     and presence bits of --colors; in front the colours and the components by floor(log2(segments)).  Needs -k and -s.\n"
			"     With --gpu the components are found on the device.  Goes with --colors, --bubbles or --distances of the same colours\n"
			"     (one walk for all; this table is written last); not with --links, --compact or --text.\n\n"
			"   --components-out <file name>\n     with --components: write the table there instead of to the standard output\n\n"
			"   --components-members <file name>\n     with --components: also write the component of every segment there, one line per segment\n\n"
			"   --superbubbles <file|sequence>\n     instead of -f: the superbubbles of the graph as TSV of integers -- the places where the paths that leave one side of a\n"
			"     segment (the entrance) meet again at one side of another (the exit) and touch nothing else: three alleles, substitutions\n"
			"     closer than k, a substitution beside an indel, nested ones each at its own entrance, and the simple bubbles.  Per row the\n"
			"     entrance and the exit as name and strand, the sides inside, the arcs, the paths, the smallest and largest path weight\n"
			"     in edges ((k+1)-mers), the number of colours and the presence bits of --colors over the inside; in front the colours and\n"
			"     the rows by their inside.  Needs -k and -s.  With --gpu they are found on the device.  Goes with --colors, --bubbles,\n"
			"     --distances or --components of the same colours (one walk for all; this table is written last); not with --links,\n"
			"     --compact or --text.\n\n"
			"   --superbubbles-out <file name>\n     with --superbubbles: write the table there instead of to the standard output\n\n"
			"   --superbubbles-members <file name>\n     with --superbubbles: also write the inside sides of every row there, one line per side\n\n"
			"   --superbubbles-max <integer>\n     with --superbubbles: the largest inside reported, 2 .. 62 (default 62)\n\n"
			"   --anchors <file|sequence>\n     instead of -f: the anchor blocks against a reference colour as TSV -- every segment that occurs exactly once in the\n"
			"     reference and exactly once in another colour is an anchor, anchors that follow each other in both are chained into maximal\n"
			"     collinear blocks: exact matches, or exact reverse-complement matches, between two intervals.  Per block the colour, the\n"
			"     reference sequence and interval, the strand, the query sequence and interval and the number of anchors; in front the\n"
			"     colours, the input sequences and per colour the blocks, anchors, edges and reverse edges it shares with the reference.\n"
			"     Needs -k and -s.  With --gpu they are found on the device.  Goes with --colors, --bubbles, --distances, --components or\n"
			"     --superbubbles of the same colours (one walk for all; this table is written last); not with --links, --compact or --text.\n\n"
			"   --locate <file|sequence>\n     instead of -f: every (k+1)-mer of the records of the --locate-in files looked up in the graph -- per query record its\n"
			"     valid windows, those found, those found on the forward strand, the runs they form and, per colour, the hits in segments of\n"
			"     that colour, as TSV; the colours as of --colors.  Beside the other tables of the same colours it is written last.\n\n"
			"   --locate-in <file name>  (accepted multiple times)\n     with --locate: a FASTA file of query records\n\n"
			"   --locate-out <file name>\n     with --locate: write the table there instead of to the standard output\n\n"
			"   --locate-walks <file name>\n     with --locate: also write the runs there, one line per run: the query's interval and the segment's\n\n"
			"   --anchors-ref <integer>\n     with --anchors: the index of the reference colour (default 0)\n\n"
			"   --anchors-out <file name>\n     with --anchors: write the table there instead of to the standard output\n\n"
			"   --anchors-paf <file name>\n     with --anchors: also write the blocks there as PAF, one line per block\n\n"
			"   <file name>\n     (required)  input file name\n\n"
			"   This utility converts the binary output of TwoPaCo to another format\n\n");
	}
}

int main(int argc, char * argv[])
{
	try
	{
		std::string binFile, format, colorsBy, colorsOut, linksOut, bubblesBy, bubblesOut, distancesBy, distancesOut, distancesPhylip, componentsBy, componentsOut, componentsMembers, superbubblesBy, superbubblesOut, superbubblesMembers, anchorsBy, anchorsOut, anchorsPaf, locateBy, locateOut, locateWalks;
		std::vector<std::string> locateIn;
		bool locateOutSet = false, locateWalksSet = false;
		std::vector<std::string> fasta;
		bool colorsOutSet = false, textSet = false, links = false, linksOutSet = false, compact = false, bubblesOutSet = false, distancesOutSet = false, distancesPhylipSet = false, componentsOutSet = false, componentsMembersSet = false, superbubblesOutSet = false, superbubblesMembersSet = false, superbubblesMaxSet = false;
		uint32_t superbubblesMax = 62, anchorsRef = 0;
		bool anchorsRefSet = false, anchorsOutSet = false, anchorsPafSet = false;
		bool prefix = false, haveK = false, haveFormat = false, haveFile = false, gpu = false, textOnDevice = false;
		int device = 0;
		size_t k = 25, threads = 16;
		bool positionalOnly = false;
		for (int i = 1; i < argc; i++)
		{
			const std::string a = argv[i];
			auto value = [&](const char * id) -> std::string
			{
				if (i + 1 >= argc) throw ArgError("Missing a value for this argument!", id);
				return argv[++i];
			};

			if (positionalOnly || a.empty() || a[0] != '-')
			{
				if (haveFile) throw ArgError("Argument already set!", "(infile)");
				binFile = a;
				haveFile = true;
			}
			else if (a == "--") positionalOnly = true;
			else if (a == "-h" || a == "--help") { Usage(); return 0; }
			else if (a == "--version") { std::printf("\n%s  version: 0.9.4\n\n", argv[0]); return 0; }
			else if (a == "--prefix") prefix = true;
			else if (a == "--gpu")
			{
				gpu = true;
				const std::string next = i + 1 < argc ? argv[i + 1] : "";
				if (!next.empty() && next.size() <= 4 && next.find_first_not_of("0123456789") == std::string::npos) device = std::atoi(argv[++i]);
			}
			else if (a == "--threads")
			{
				const std::string v = value("(--threads)");
				char * end = 0;
				const long long parsed = std::strtoll(v.c_str(), &end, 10);
				if (end == v.c_str() || *end != 0 || parsed < 1) throw ArgError("Couldn't read argument value from string '" + v + "'", "(--threads)");
				threads = size_t(std::min<long long>(parsed, 16));
			}
			else if (a == "--text")
			{
				const std::string v = value("(--text)");
				if (v != "host" && v != "device") throw ArgError("Value '" + v + "' does not meet constraint: host|device", "Argument: (--text)");
				textOnDevice = v == "device";
				textSet = true;
			}
			else if (a == "--colors")
			{
				colorsBy = value("(--colors)");
				if (colorsBy != "file" && colorsBy != "sequence") throw ArgError("Value '" + colorsBy + "' does not meet constraint: file|sequence", "Argument: (--colors)");
			}
			else if (a == "--colors-out") { colorsOut = value("(--colors-out)"); colorsOutSet = true; }
			else if (a == "--links") links = true;
			else if (a == "--links-out") { linksOut = value("(--links-out)"); linksOutSet = true; }
			else if (a == "--compact") compact = true;
			else if (a == "--bubbles")
			{
				bubblesBy = value("(--bubbles)");
				if (bubblesBy != "file" && bubblesBy != "sequence") throw ArgError("Value '" + bubblesBy + "' does not meet constraint: file|sequence", "Argument: (--bubbles)");
			}
			else if (a == "--bubbles-out") { bubblesOut = value("(--bubbles-out)"); bubblesOutSet = true; }
			else if (a == "--distances")
			{
				distancesBy = value("(--distances)");
				if (distancesBy != "file" && distancesBy != "sequence") throw ArgError("Value '" + distancesBy + "' does not meet constraint: file|sequence", "Argument: (--distances)");
			}
			else if (a == "--distances-out") { distancesOut = value("(--distances-out)"); distancesOutSet = true; }
			else if (a == "--distances-phylip") { distancesPhylip = value("(--distances-phylip)"); distancesPhylipSet = true; }
			else if (a == "--components")
			{
				componentsBy = value("(--components)");
				if (componentsBy != "file" && componentsBy != "sequence") throw ArgError("Value '" + componentsBy + "' does not meet constraint: file|sequence", "Argument: (--components)");
			}
			else if (a == "--components-out") { componentsOut = value("(--components-out)"); componentsOutSet = true; }
			else if (a == "--components-members") { componentsMembers = value("(--components-members)"); componentsMembersSet = true; }
			else if (a == "--superbubbles")
			{
				superbubblesBy = value("(--superbubbles)");
				if (superbubblesBy != "file" && superbubblesBy != "sequence") throw ArgError("Value '" + superbubblesBy + "' does not meet constraint: file|sequence", "Argument: (--superbubbles)");
			}
			else if (a == "--superbubbles-out") { superbubblesOut = value("(--superbubbles-out)"); superbubblesOutSet = true; }
			else if (a == "--superbubbles-members") { superbubblesMembers = value("(--superbubbles-members)"); superbubblesMembersSet = true; }
			else if (a == "--superbubbles-max")
			{
				const std::string v = value("(--superbubbles-max)");
				char * end = 0;
				const long n = std::strtol(v.c_str(), &end, 10);
				if (v.empty() || *end || n < 2 || n > 62) throw ArgError("Value '" + v + "' does not meet constraint: an integer 2 .. 62", "Argument: (--superbubbles-max)");
				superbubblesMax = uint32_t(n);
				superbubblesMaxSet = true;
			}
			else if (a == "--anchors")
			{
				anchorsBy = value("(--anchors)");
				if (anchorsBy != "file" && anchorsBy != "sequence") throw ArgError("Value '" + anchorsBy + "' does not meet constraint: file|sequence", "Argument: (--anchors)");
			}
			else if (a == "--locate")
			{
				locateBy = value("(--locate)");
				if (locateBy != "file" && locateBy != "sequence") throw ArgError("Value '" + locateBy + "' does not meet constraint: file|sequence", "Argument: (--locate)");
			}
			else if (a == "--locate-in") locateIn.push_back(value("(--locate-in)"));
			else if (a == "--locate-out") { locateOut = value("(--locate-out)"); locateOutSet = true; }
			else if (a == "--locate-walks") { locateWalks = value("(--locate-walks)"); locateWalksSet = true; }
			else if (a == "--anchors-out") { anchorsOut = value("(--anchors-out)"); anchorsOutSet = true; }
			else if (a == "--anchors-paf") { anchorsPaf = value("(--anchors-paf)"); anchorsPafSet = true; }
			else if (a == "--anchors-ref")
			{
				const std::string v = value("(--anchors-ref)");
				char * end = 0;
				const long long n = std::strtoll(v.c_str(), &end, 10);
				if (v.empty() || *end || n < 0 || n > 0x7FFFFFFFll) throw ArgError("Value '" + v + "' does not meet constraint: a colour index", "Argument: (--anchors-ref)");
				anchorsRef = uint32_t(n);
				anchorsRefSet = true;
			}
			else if (a == "-k" || a == "--kvalue")
			{
				const std::string v = value("(--kvalue)");
				char * end = 0;
				const long long parsed = std::strtoll(v.c_str(), &end, 10);
				if (end == v.c_str() || *end != 0 || parsed < 0) throw ArgError("Couldn't read argument value from string '" + v + "'", "(--kvalue)");
				k = size_t(parsed);
				haveK = true;
			}
			else if (a == "-s" || a == "--seqfile") fasta.push_back(value("(--seqfile)"));
			else if (a == "-f" || a == "--format")
			{
				format = value("(--format)");
				static const char * allowed[] = {"seq", "group", "dot", "gfa1", "gfa2", "fasta"};
				if (std::find(allowed, allowed + 6, format) == allowed + 6) throw ArgError("Value '" + format + "' does not meet constraint: seq|group|dot|gfa1|gfa2|fasta", "Argument: -f (--format)");
				haveFormat = true;
			}
			else throw ArgError("Couldn't find match for argument", "(" + a + ")");
		}

		const bool colors = !colorsBy.empty(), bubbles = !bubblesBy.empty(), distances = !distancesBy.empty(), components = !componentsBy.empty();
		const bool superbubbles = !superbubblesBy.empty();
		const bool anchors = !anchorsBy.empty();
		const bool locate = !locateBy.empty();
		if (locate && haveFormat) throw ArgError("Mutually exclusive argument already set!", "(--locate)");
		if (locate && colors && colorsBy != locateBy) throw ArgError("The locate table and the colour table share one set of colours: --colors " + colorsBy + " does not go with --locate " + locateBy, "(--locate)");
		if (locate && bubbles && bubblesBy != locateBy) throw ArgError("The locate table and the bubble table share one set of colours: --bubbles " + bubblesBy + " does not go with --locate " + locateBy, "(--locate)");
		if (locate && distances && distancesBy != locateBy) throw ArgError("The locate table and the distance table share one set of colours: --distances " + distancesBy + " does not go with --locate " + locateBy, "(--locate)");
		if (locate && components && componentsBy != locateBy) throw ArgError("The locate table and the component table share one set of colours: --components " + componentsBy + " does not go with --locate " + locateBy, "(--locate)");
		if (locate && superbubbles && superbubblesBy != locateBy) throw ArgError("The locate table and the superbubble table share one set of colours: --superbubbles " + superbubblesBy + " does not go with --locate " + locateBy, "(--locate)");
		if (locate && anchors && anchorsBy != locateBy) throw ArgError("The locate table and the anchor table share one set of colours: --anchors " + anchorsBy + " does not go with --locate " + locateBy, "(--locate)");
		if (locate && links) throw ArgError("The locate table and the link table are written one at a time: not with --links", "(--locate)");
		if (locate && compact) throw ArgError("The locate table and the compact text are written one at a time: not with --compact", "(--locate)");
		if (locate && textSet) throw ArgError("The locate table is formatted by the host: not with --locate", "(--text)");
		if (locate && locateIn.empty()) throw ArgError("The locate table needs a query: --locate-in <fasta file>", "(--locate)");
		if (!locateIn.empty() && !locate) throw ArgError("This argument needs --locate <file|sequence>", "(--locate-in)");
		if (locateOutSet && !locate) throw ArgError("This argument needs --locate <file|sequence>", "(--locate-out)");
		if (locateWalksSet && !locate) throw ArgError("This argument needs --locate <file|sequence>", "(--locate-walks)");
		if (locateWalksSet && locateWalks.empty()) throw ArgError("The locate walks need a file name", "(--locate-walks)");
		if (anchors && haveFormat) throw ArgError("Mutually exclusive argument already set!", "(--anchors)");
		if (anchors && colors && colorsBy != anchorsBy) throw ArgError("The anchor table and the colour table share one set of colours: --colors " + colorsBy + " does not go with --anchors " + anchorsBy, "(--anchors)");
		if (anchors && bubbles && bubblesBy != anchorsBy) throw ArgError("The anchor table and the bubble table share one set of colours: --bubbles " + bubblesBy + " does not go with --anchors " + anchorsBy, "(--anchors)");
		if (anchors && distances && distancesBy != anchorsBy) throw ArgError("The anchor table and the distance table share one set of colours: --distances " + distancesBy + " does not go with --anchors " + anchorsBy, "(--anchors)");
		if (anchors && components && componentsBy != anchorsBy) throw ArgError("The anchor table and the component table share one set of colours: --components " + componentsBy + " does not go with --anchors " + anchorsBy, "(--anchors)");
		if (anchors && superbubbles && superbubblesBy != anchorsBy) throw ArgError("The anchor table and the superbubble table share one set of colours: --superbubbles " + superbubblesBy + " does not go with --anchors " + anchorsBy, "(--anchors)");
		if (anchors && links) throw ArgError("The anchor table and the link table are written one at a time: not with --links", "(--anchors)");
		if (anchors && compact) throw ArgError("The anchor table and the compact text are written one at a time: not with --compact", "(--anchors)");
		if (anchors && textSet) throw ArgError("The anchor table is formatted by the host: not with --anchors", "(--text)");
		if (anchorsOutSet && !anchors) throw ArgError("This argument needs --anchors <file|sequence>", "(--anchors-out)");
		if (anchorsPafSet && !anchors) throw ArgError("This argument needs --anchors <file|sequence>", "(--anchors-paf)");
		if (anchorsRefSet && !anchors) throw ArgError("This argument needs --anchors <file|sequence>", "(--anchors-ref)");
		if (anchorsPafSet && anchorsPaf.empty()) throw ArgError("The anchor PAF needs a file name", "(--anchors-paf)");
		if (superbubbles && haveFormat) throw ArgError("Mutually exclusive argument already set!", "(--superbubbles)");
		if (superbubbles && colors && colorsBy != superbubblesBy) throw ArgError("The superbubble table and the colour table share one set of colours: --colors " + colorsBy + " does not go with --superbubbles " + superbubblesBy, "(--superbubbles)");
		if (superbubbles && bubbles && bubblesBy != superbubblesBy) throw ArgError("The superbubble table and the bubble table share one set of colours: --bubbles " + bubblesBy + " does not go with --superbubbles " + superbubblesBy, "(--superbubbles)");
		if (superbubbles && distances && distancesBy != superbubblesBy) throw ArgError("The superbubble table and the distance table share one set of colours: --distances " + distancesBy + " does not go with --superbubbles " + superbubblesBy, "(--superbubbles)");
		if (superbubbles && components && componentsBy != superbubblesBy) throw ArgError("The superbubble table and the component table share one set of colours: --components " + componentsBy + " does not go with --superbubbles " + superbubblesBy, "(--superbubbles)");
		if (superbubbles && links) throw ArgError("The superbubble table and the link table are written one at a time: not with --links", "(--superbubbles)");
		if (superbubbles && compact) throw ArgError("The superbubble table and the compact text are written one at a time: not with --compact", "(--superbubbles)");
		if (superbubbles && textSet) throw ArgError("The superbubble table is formatted by the host: not with --superbubbles", "(--text)");
		if (superbubblesOutSet && !superbubbles) throw ArgError("This argument needs --superbubbles <file|sequence>", "(--superbubbles-out)");
		if (superbubblesMembersSet && !superbubbles) throw ArgError("This argument needs --superbubbles <file|sequence>", "(--superbubbles-members)");
		if (superbubblesMaxSet && !superbubbles) throw ArgError("This argument needs --superbubbles <file|sequence>", "(--superbubbles-max)");
		if (superbubblesMembersSet && superbubblesMembers.empty()) throw ArgError("The superbubble members need a file name", "(--superbubbles-members)");
		if (components && haveFormat) throw ArgError("Mutually exclusive argument already set!", "(--components)");
		if (components && colors && colorsBy != componentsBy) throw ArgError("The component table and the colour table share one set of colours: --colors " + colorsBy + " does not go with --components " + componentsBy, "(--components)");
		if (components && bubbles && bubblesBy != componentsBy) throw ArgError("The component table and the bubble table share one set of colours: --bubbles " + bubblesBy + " does not go with --components " + componentsBy, "(--components)");
		if (components && distances && distancesBy != componentsBy) throw ArgError("The component table and the distance table share one set of colours: --distances " + distancesBy + " does not go with --components " + componentsBy, "(--components)");
		if (components && links) throw ArgError("The component table and the link table are written one at a time: not with --links", "(--components)");
		if (components && compact) throw ArgError("The component table and the compact text are written one at a time: not with --compact", "(--components)");
		if (components && textSet) throw ArgError("The component table is formatted by the host: not with --components", "(--text)");
		if (componentsOutSet && !components) throw ArgError("This argument needs --components <file|sequence>", "(--components-out)");
		if (componentsMembersSet && !components) throw ArgError("This argument needs --components <file|sequence>", "(--components-members)");
		if (componentsMembersSet && componentsMembers.empty()) throw ArgError("The component members need a file name", "(--components-members)");
		if (distances && haveFormat) throw ArgError("Mutually exclusive argument already set!", "(--distances)");
		// one set of colours per run: the modes are compared before anything else is said about the combination
		if (distances && colors && colorsBy != distancesBy) throw ArgError("The distance table and the colour table share one set of colours: --colors " + colorsBy + " does not go with --distances " + distancesBy, "(--distances)");
		if (distances && bubbles && bubblesBy != distancesBy) throw ArgError("The distance table and the bubble table share one set of colours: --bubbles " + bubblesBy + " does not go with --distances " + distancesBy, "(--distances)");
		if (distances && links) throw ArgError("The distance table and the link table are written one at a time: not with --links", "(--distances)");
		if (distances && compact) throw ArgError("The distance table and the compact text are written one at a time: not with --compact", "(--distances)");
		if (distances && textSet) throw ArgError("The distance table is formatted by the host: not with --distances", "(--text)");
		if (distancesOutSet && !distances) throw ArgError("This argument needs --distances <file|sequence>", "(--distances-out)");
		if (distancesPhylipSet && !distances) throw ArgError("This argument needs --distances <file|sequence>", "(--distances-phylip)");
		if (distancesPhylipSet && distancesPhylip.empty()) throw ArgError("The PHYLIP matrix needs a file name", "(--distances-phylip)");
		if (bubbles && haveFormat) throw ArgError("Mutually exclusive argument already set!", "(--bubbles)");
		if (bubbles && colors) throw ArgError("The bubble table and the colour table are written one at a time: not with --colors", "(--bubbles)");
		if (bubbles && links) throw ArgError("The bubble table and the link table are written one at a time: not with --links", "(--bubbles)");
		if (bubbles && compact) throw ArgError("The bubble table and the compact text are written one at a time: not with --compact", "(--bubbles)");
		if (bubbles && textSet) throw ArgError("The bubble table is formatted by the host: not with --bubbles", "(--text)");
		if (bubblesOutSet && !bubbles) throw ArgError("This argument needs --bubbles <file|sequence>", "(--bubbles-out)");
		if (colors && haveFormat) throw ArgError("Mutually exclusive argument already set!", "(--colors)");
		if (colors && textSet) throw ArgError("The colour table is formatted by the host: not with --colors", "(--text)");
		if (colorsOutSet && !colors) throw ArgError("This argument needs --colors <file|sequence>", "(--colors-out)");
		if (links && haveFormat) throw ArgError("Mutually exclusive argument already set!", "(--links)");
		if (links && colors) throw ArgError("The link table and the colour table are written one at a time: not with --colors", "(--links)");
		if (links && textSet) throw ArgError("The link table is formatted by the host: not with --links", "(--text)");
		if (linksOutSet && !links) throw ArgError("This argument needs --links", "(--links-out)");
		if (compact && format != "gfa1") throw ArgError("The compact text is gfa1 with every link once: it needs -f gfa1", "(--compact)");
		if (compact && textOnDevice) throw ArgError("The compact text is formatted by the host: not with --text device", "(--compact)");
		if (!haveK) throw ArgError("Required argument missing: kvalue", " ");
		if (!haveFormat && !colors && !links && !bubbles && !distances && !components && !superbubbles && !anchors && !locate) throw ArgError("Required argument missing: format", " ");
		if (!haveFile) throw ArgError("Required argument missing: infile", " ");
		if (textOnDevice && !gpu) throw ArgError("Value 'device' does not meet constraint: the text is rendered on the device only with --gpu", "Argument: (--text)");
		const bool needsSequences = colors || links || bubbles || distances || components || superbubbles || anchors || locate || format == "gfa1" || format == "gfa2" || format == "fasta";
		if (needsSequences && fasta.empty()) throw ArgError("Required argument missing\n", "Argument: seqfilename");

		DumpStats stats;
		std::unique_ptr<DeviceLibrary> lib;
		if (gpu && needsSequences) lib.reset(new DeviceLibrary(device));  // before the first byte of output: no device is an error
		stats.threads = lib ? threads : 1;
		const bool deviceText = lib && textOnDevice;
		stats.text = deviceText ? "device" : "host";
		Out out(!deviceText && !compact);  // --text device, --compact: the header lines wait until the table is known to be good
		// --distances beside --colors or --bubbles (the same colours, checked above): that table's walk or segment build and its
		// colour table serve the distance table too, which is written after it
		DistancesWanted also;
		also.on = distances && (colors || bubbles);
		also.out = distancesOut;
		also.phylip = distancesPhylip;
		AnchorsWanted anchorsTo;
		anchorsTo.on = anchors;
		anchorsTo.ref = anchorsRef;
		anchorsTo.out = anchorsOut;
		anchorsTo.paf = anchorsPaf;
		LocateWanted locateTo;
		locateTo.on = locate;
		locateTo.in = locateIn;
		locateTo.out = locateOut;
		locateTo.walks = locateWalks;
		if ((colors || links || bubbles || distances || components || superbubbles || anchors || locate) && lib)
		{
			std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
			InputSequences seq;
			LoadedSequences loaded;
			LoadSequences(fasta, prefix, threads, seq, loaded);
			stats.loadMs = MsSince(t0);
			TablesWanted want;
			want.colors = colors;
			want.links = links;
			want.bubbles = bubbles;
			want.distances = distances;
			want.components = components;
			want.superbubbles = superbubbles;
			want.superbubblesOut = superbubblesOut;
			want.superbubblesMembers = superbubblesMembers;
			want.superbubblesMax = superbubblesMax;
			want.anchors = anchorsTo;
			want.locate = locateTo;
			want.bySequence = (colors ? colorsBy : bubbles ? bubblesBy : distances ? distancesBy : components ? componentsBy : superbubbles ? superbubblesBy : anchors ? anchorsBy : locateBy) == "sequence";
			want.componentsOut = componentsOut;
			want.componentsMembers = componentsMembers;
			want.out = colors ? colorsOut : links ? linksOut : bubblesOut;
			want.distancesOut = distancesOut;
			want.distancesPhylip = distancesPhylip;
			DumpTablesOnDevice(*lib, binFile, fasta, k, threads, seq, loaded, want, stats);
		}
		else if (components || superbubbles || anchors || locate)
		{
			ComponentsWanted wanted;
			wanted.on = components;
			wanted.out = componentsOut;
			wanted.members = componentsMembers;
			SuperbubblesWanted super;
			super.on = superbubbles;
			super.out = superbubblesOut;
			super.members = superbubblesMembers;
			super.maxInside = superbubblesMax;
			DumpComponents(binFile, fasta, k, prefix, (components ? componentsBy : superbubbles ? superbubblesBy : anchors ? anchorsBy : locateBy) == "sequence", wanted, colors, bubbles, colors ? colorsOut : bubblesOut, distances, also, super, anchorsTo, locateTo);
		}
		else if (colors) DumpColors(binFile, fasta, k, prefix, colorsBy == "sequence", colorsOut, also);
		else if (links) DumpLinks(binFile, fasta, k, prefix, linksOut);
		else if (bubbles) DumpBubbles(binFile, fasta, k, prefix, bubblesBy == "sequence", bubblesOut, also);
		else if (distances) DumpDistances(binFile, fasta, k, prefix, distancesBy == "sequence", distancesOut, distancesPhylip);
		else if (lib)
		{
			// the serial branch below, with the walk's serial part done on the device
			std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
			InputSequences seq;
			LoadedSequences loaded;
			if (format == "gfa1") out << "H\tVN:Z:1.0\n";
			if (format == "gfa2") out << "H\tVN:Z:2.0\n";
			LoadSequences(fasta, format == "fasta" ? true : prefix, threads, seq, loaded);
			stats.loadMs = MsSince(t0);
			if (format == "gfa1" && !compact)
			{
				for (const std::string & name : seq.name) out << "S\t" << name << "\t*\tUR:Z:" << seq.file[name] << '\n';
			}

			DumpSegmentsOnDevice(*lib, binFile, fasta, k, threads, format, seq, loaded, out, stats, deviceText, compact);
		}
		else if (format == "seq") DumpSeq(binFile, out);
		else if (format == "group") DumpGroups(binFile, out);
		else if (format == "dot") DumpDot(binFile, out);
		else if (compact) DumpCompact(binFile, fasta, k, prefix);
		else
		{
			InputSequences seq;
			if (format == "gfa1")
			{
				out << "H\tVN:Z:1.0\n";
				ListSequences(fasta, prefix, seq);
				for (const std::string & name : seq.name) out << "S\t" << name << "\t*\tUR:Z:" << seq.file[name] << '\n';
				Gfa1Sink sink(out, seq);
				WalkSegments(binFile, fasta, k, sink);
			}
			else if (format == "gfa2")
			{
				out << "H\tVN:Z:2.0\n";
				ListSequences(fasta, prefix, seq);
				Gfa2Sink sink(out, seq);
				WalkSegments(binFile, fasta, k, sink);
			}
			else
			{
				ListSequences(fasta, true, seq);
				FastaSink sink(out);
				WalkSegments(binFile, fasta, k, sink);
			}
		}

		stats.Write();
	}
	catch (ArgError & e)
	{
		std::fflush(stdout);
		if (e.arg == "Argument: seqfilename")
		{
			std::fprintf(stderr, "error: %s for arg %s\n", e.what.c_str(), e.arg.c_str());  // thrown after parsing, graphdump.cpp:669-693
		}
		else
		{
			std::fprintf(stderr, "PARSE ERROR: %s\n             %s\n\nBrief USAGE: \n   %s  [-k <integer>] [-s <string>] ... -f <seq|group|dot|gfa1|gfa2|fasta> [--prefix] [--] [--version] [-h] <file name>\n\n"
				"For complete USAGE and HELP type: \n   %s --help\n\n", e.arg.c_str(), e.what.c_str(), argv[0], argv[0]);
		}

		return 1;
	}
	catch (std::runtime_error & e)
	{
		std::fflush(stdout);
		std::fprintf(stderr, "error: %s\n", e.what());
		return 1;
	}

	return 0;
}
