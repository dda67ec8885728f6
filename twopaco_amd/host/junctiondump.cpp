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
//             |  --classes file|sequence [--classes-out <path>] [--classes-members <path>]
//             |  --tracks file|sequence [--tracks-of <colour>] [--tracks-out <path>] [--tracks-bedgraph <path>]
//             |  --variants file|sequence [--variants-ref <colour>] [--variants-out <path>] [--variants-vcf <path>] [--superbubbles-max <n>]
//             (the last ten instead of -f)
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
// --classes file|sequence [--classes-out <path>] [--classes-members <path>] (an addition; instead of -f): the colour classes -- the
// distinct sets of colours that segments have, and per class its segments, bases, edges and occurrences; include/twopaco_hip.h
// defines them -- as TSV of integers (graphformat.h: WriteClasses) and, asked for, the class of every segment (WriteClassMembers).
// Without --gpu the serial walk, then ComputeColors and ComputeClasses; with --gpu the colour stage and the class stage over one
// segment build (csrc/tpc_classes.hip); the bytes are the same.  It goes with what --colors goes with, and with --colors, of the
// same colours, and is written after every other table but the track table; not with -f, --links, --bubbles or --text.
// --tracks file|sequence [--tracks-of <colour>] [--tracks-out <path>] [--tracks-bedgraph <path>] (an addition; instead of -f): the
// presence tracks -- for every stretch of every input sequence the colours that share it, neighbouring occurrences of equal presence
// merged into one interval; include/twopaco_hip.h defines them -- as TSV of integers (graphformat.h: WriteTracks) and, asked for, as
// bedGraph of the number of colours (WriteTracksBedGraph).  Without --gpu the serial walk, then ComputeColors and ComputeTracks; with
// --gpu the colour stage and the track stage over one segment build (csrc/tpc_tracks.hip); the bytes are the same.  It goes with
// what --classes goes with, and with --classes, of the same colours, and is written after every other table but the variant table;
// not with -f, --links, --bubbles or --text.
// --variants file|sequence [--variants-ref <colour>] [--variants-out <path>] [--variants-vcf <path>] (an addition; instead of -f): the
// alleles every genome walks through every superbubble -- include/twopaco_hip.h defines walk, traversal, allele and site -- as TSV of
// integers (graphformat.h: WriteVariants) and, with a reference colour, as VCF 4.2 (WriteVariantsVcf).  Without --gpu the serial walk,
// then ComputeColors, ComputeLinks, ComputeSuperbubbles and ComputeVariants; with --gpu the colour, link, superbubble and variant stages
// over one segment build (csrc/tpc_variants.hip); the bytes are the same.  It goes with what --tracks goes with, and with --tracks, of
// the same colours, and is written last; not with -f, --links, --bubbles or --text.
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

	// ---------------------------------------------------------------------------------------- the tables and --compact, serial
	struct SerialTable
	{
		InputSequences seq;
		LoadedSequences loaded;
		EventCollector events;
		std::vector<uint32_t> seqEventBegin;
		EventTable table;
	};

	// the walk's event table; nothing is printed before it is complete
	void WalkTable(const std::string & binFile, const std::vector<std::string> & fasta, size_t k, bool prefix, bool bodies, SerialTable & out)
	{
		if (bodies) LoadSequences(fasta, prefix, 1, out.seq, out.loaded);
		else ListSequences(fasta, prefix, out.seq);
		WalkSegments(binFile, fasta, k, out.events);
		out.events.Table(out.seq.name.size(), out.seqEventBegin, out.table);
	}

	void DumpCompact(const std::string & binFile, const std::vector<std::string> & fasta, size_t k, bool prefix)
	{
		SerialTable t;
		WalkTable(binFile, fasta, k, prefix, true, t);
		LinkTable links;
		ComputeLinks(t.table, links);
		t.table.linkFirst = links.linkFirst.data();
		Out head(false);
		HeaderLines("gfa1", t.seq, head, true);
		std::fwrite(head.Text().data(), 1, head.Text().size(), stdout);
		FormatEvents(t.table, t.seq, t.loaded, k, "gfa1", 1, -1, 0);
	}

	// The colours of a request, once the input's files and sequences are known; the reference colour of --anchors must be one of them
	void MakeRequestColors(const TableRequest & request, const InputSequences & seq, const std::vector<std::string> & fasta, ColorMap & map)
	{
		if (!NeedsColorMap(request)) return;
		MakeColorMap(seq, fasta, request.bySequence, map);
		if (request.On(ANCHORS) && request.anchorsRef >= map.label.size())
		{
			throw ArgError("Value '" + std::to_string(request.anchorsRef) + "' does not meet constraint: a colour index below " + std::to_string(map.label.size()), "Argument: (--anchors-ref)");
		}

		if (request.On(TRACKS) && request.tracksOf != TrackTable::ALL && request.tracksOf >= map.label.size())
		{
			throw ArgError("Value '" + std::to_string(request.tracksOf) + "' does not meet constraint: a colour index below " + std::to_string(map.label.size()), "Argument: (--tracks-of)");
		}

		if (request.On(VARIANTS) && request.variantsRef != VariantTable::NONE && request.variantsRef >= map.label.size())
		{
			throw ArgError("Value '" + std::to_string(request.variantsRef) + "' does not meet constraint: a colour index below " + std::to_string(map.label.size()), "Argument: (--variants-ref)");
		}
	}

	// A table request, serial: one walk (with the letters when the edge index reads them), the serial statements the request needs,
	// then the tables in their order.  A stream the walk refuses prints the walk's error and nothing else.
	void DumpTables(const std::string & binFile, const std::vector<std::string> & fasta, size_t k, bool prefix, const TableRequest & request)
	{
		SerialTable t;
		WalkTable(binFile, fasta, k, prefix, NeedsLetters(request), t);
		Tables tables;
		MakeRequestColors(request, t.seq, fasta, tables.map);
		LoadQueries(request, 1, tables);
		if (NeedsLetters(request)) tables.letters = &t.loaded;
		ComputeTables(t.table, t.loaded, k, request, tables);
		WriteTables(COLORS, t.table, k, request, t.seq, tables, [](int) {});
	}

	// Positions of packed query text per device call, whole records: 2^28, or what TWOPACO_LOCATE_BATCH says (tests: a small query in
	// several batches)
	uint64_t LocateBatchPositions()
	{
		const char * e = std::getenv("TWOPACO_LOCATE_BATCH");
		const long long n = e && *e ? std::atoll(e) : 0;
		return n > 0 ? uint64_t(n) : uint64_t(1) << 28;
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
		double loadMs, packMs, deviceMs, kernelMs, indexMs, formatMs, textKernelMs;
		double stageMs[TABLES + 1], stageKernelMs[TABLES + 1];  // of the stages of BuildTables: the tables', and EDGES
		uint64_t links, linkOccurrences, bubbles, components, largestComponent, superbubbles, superbubbleMembers, superbubblesUnmirrored, anchorBlocks, anchors;
		uint64_t locateRuns, locateBatches, classes, largestClass, trackIntervals, variantAlleles;
		size_t threads;
		DumpStats() : path("host"), text("host"), events(0), segments(0), nNamed(0), deviceBytes(0), streamBytes(0), textBytes(0), tableBytes(0), loadMs(0), packMs(0),
			deviceMs(0), kernelMs(0), indexMs(0), formatMs(0), textKernelMs(0), stageMs(), stageKernelMs(), links(0), linkOccurrences(0), bubbles(0), components(0), largestComponent(0),
			superbubbles(0), superbubbleMembers(0), superbubblesUnmirrored(0), anchorBlocks(0), anchors(0), locateRuns(0), locateBatches(0), classes(0), largestClass(0), trackIntervals(0), variantAlleles(0), threads(1) {}

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
				"\"edges_kernel_ms\": %.3f, \"edges_ms\": %.3f, \"locate_kernel_ms\": %.3f, \"locate_ms\": %.3f, \"locate_runs\": %llu, \"locate_batches\": %llu, "
				"\"classes_kernel_ms\": %.3f, \"classes_ms\": %.3f, \"classes\": %llu, \"largest_class\": %llu, "
				"\"tracks_kernel_ms\": %.3f, \"tracks_ms\": %.3f, \"track_intervals\": %llu, "
				"\"variants_kernel_ms\": %.3f, \"variants_ms\": %.3f, \"variant_alleles\": %llu}\n", path.c_str(), (unsigned long long)events, (unsigned long long)segments, (unsigned long long)nNamed, deviceMs, kernelMs, loadMs,
				packMs, indexMs, formatMs, (unsigned long long)threads, (unsigned long long)deviceBytes, (unsigned long long)streamBytes, (unsigned long long)textBytes,
				(unsigned long long)tableBytes, text.c_str(), textKernelMs, stageKernelMs[COLORS], stageMs[COLORS], stageKernelMs[LINKS], stageMs[LINKS], (unsigned long long)links,
				(unsigned long long)linkOccurrences, stageKernelMs[BUBBLES], stageMs[BUBBLES], (unsigned long long)bubbles, stageKernelMs[DISTANCES], stageMs[DISTANCES],
				stageKernelMs[COMPONENTS], stageMs[COMPONENTS], (unsigned long long)components, (unsigned long long)largestComponent, stageKernelMs[SUPERBUBBLES],
				stageMs[SUPERBUBBLES], (unsigned long long)superbubbles, (unsigned long long)superbubbleMembers, (unsigned long long)superbubblesUnmirrored, stageKernelMs[ANCHORS],
				stageMs[ANCHORS], (unsigned long long)anchorBlocks, (unsigned long long)anchors, stageKernelMs[EDGES], stageMs[EDGES], stageKernelMs[LOCATE], stageMs[LOCATE],
				(unsigned long long)locateRuns, (unsigned long long)locateBatches, stageKernelMs[CLASSES], stageMs[CLASSES], (unsigned long long)classes,
				(unsigned long long)largestClass, stageKernelMs[TRACKS], stageMs[TRACKS], (unsigned long long)trackIntervals, stageKernelMs[VARIANTS],
				stageMs[VARIANTS], (unsigned long long)variantAlleles);
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

	const char * const PACKER_DISAGREES = "--gpu: the packer and the parser disagree about the input sequences";

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
		const std::vector<uint64_t> ambiguous = AmbiguousPositions(text, loaded, PACKER_DISAGREES);
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

	// graphdump's clock around the stages of BuildTables: DumpStats and the [timing] lines (the colour table's comes last, after the files)
	const char * const STAGE_TIMING[TABLES + 1] = {0, "link table", "bubble table", "distance matrices", "component table", "superbubble table", "anchor table", "locate", "class table", "track table", "variant table", "edge index"};
	const StageWording GPU_WORDING = {"--gpu: the ", "colour map"};

	void BuildTablesTimed(DeviceLibrary & lib, const TableRequest & request, const uint64_t * counts, bool linkBits, Tables & tables, DumpStats & stats)
	{
		std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
		auto close = [&](int stage)
		{
			stats.stageMs[stage] = MsSince(last);
			last = std::chrono::steady_clock::now();
			if (STAGE_TIMING[stage]) TimingLine(STAGE_TIMING[stage], stats.stageMs[stage], stats.stageKernelMs[stage]);
		};

		StageObserver observer;
		observer.built = [&](int stage, int kernel)
		{
			stats.stageKernelMs[stage] = stage == LOCATE ? observer.locateKernelMs : lib.kernel_ms(lib.ctx, kernel);
			if (stage == EDGES) close(stage);
		};
		observer.fetched = close;
		BuildTables(lib, request, STAGES_DISTANCES_FIRST, counts, linkBits, LocateBatchPositions(), GPU_WORDING, tables, observer);
		stats.links = tables.linkRows;
		stats.linkOccurrences = tables.links.occurrences;
		stats.bubbles = tables.bubbles.source.size();
		stats.components = tables.components.Rows();
		stats.largestComponent = tables.components.Largest();
		stats.superbubbles = tables.superbubbles.Rows();
		stats.superbubbleMembers = tables.superbubbles.members.size();
		stats.superbubblesUnmirrored = tables.superbubbles.unmirrored;
		stats.anchorBlocks = tables.anchors.Rows();
		stats.anchors = tables.anchors.Anchors();
		stats.locateRuns = tables.locate.Runs();
		stats.locateBatches = observer.locateBatches;
		stats.classes = tables.classes.Rows();
		stats.largestClass = tables.classes.Largest();
		stats.trackIntervals = tables.tracks.Rows();
		stats.variantAlleles = tables.variants.Alleles();
	}

	// A table request with --gpu: one segment build, the table stays on the device, and the stages that are wanted run there
	// (devicegraph.h: BuildTables).  Fetched is what the files print and no more: the event table for the names and lengths of any
	// rows; --distances alone fetches the two matrices, neither colour rows nor event table.
	void DumpTablesOnDevice(DeviceLibrary & lib, const std::string & binFile, const std::vector<std::string> & fasta, size_t k, size_t threads,
		const InputSequences & seq, const LoadedSequences & loaded, const TableRequest & request, DumpStats & stats)
	{
		uint64_t counts[6] = {0, 0, 0, 0, 0, 0};
		size_t sequences = 0;
		std::chrono::steady_clock::time_point t0;
		BuildTableOnDevice(lib, binFile, fasta, k, threads, loaded, stats, counts, sequences, t0);
		Tables tables;
		MakeRequestColors(request, seq, fasta, tables.map);
		if (NeedsColorMap(request) && tables.map.colorOfSequence.size() != sequences) throw std::runtime_error(PACKER_DISAGREES);
		LoadQueries(request, threads, tables);
		tables.letters = &loaded;
		BuildTablesTimed(lib, request, counts, false, tables, stats);
		Events held(counts[0], sequences);
		if (NeedsEventTable(request)) FetchTable(lib, held);
		stats.deviceMs = MsSince(t0);
		t0 = std::chrono::steady_clock::now();
		WriteTables(COLORS, held.table, k, request, seq, tables, [](int) {});
		stats.formatMs = MsSince(t0);
		if (request.On(COLORS)) TimingLine("colour table", stats.stageMs[COLORS], stats.stageKernelMs[COLORS]);
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
		Tables tables;
		if (compact)
		{
			BuildTablesTimed(lib, TableRequest(), counts, true, tables, stats);
			table.linkFirst = tables.links.linkFirst.data();
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
		std::printf("\nUSAGE: \n\n   graphdump  [-k <integer>] [-s <string>] ... -f <seq|group|dot|gfa1|gfa2|fasta> [--prefix] [--gpu [<device>]] [--threads <integer>] [--text <host|device>] [--colors <file|sequence>] [--colors-out <file name>] [--links] [--links-out <file name>] [--compact] [--bubbles <file|sequence>] [--bubbles-out <file name>] [--distances <file|sequence>] [--distances-out <file name>] [--distances-phylip <file name>] [--components <file|sequence>] [--components-out <file name>] [--components-members <file name>] [--superbubbles <file|sequence>] [--superbubbles-out <file name>] [--superbubbles-members <file name>] [--superbubbles-max <integer>] [--anchors <file|sequence>] [--anchors-ref <integer>] [--anchors-out <file name>] [--anchors-paf <file name>] [--classes <file|sequence>] [--classes-out <file name>] [--classes-members <file name>] [--tracks <file|sequence>] [--tracks-of <integer>] [--tracks-out <file name>] [--tracks-bedgraph <file name>] [--variants <file|sequence>] [--variants-ref <integer>] [--variants-out <file name>] [--variants-vcf <file name>] [--] [--version] [-h] <file name>\n\n"
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
			"   --classes <file|sequence>\n     instead of -f: the colour classes of the graph as TSV of integers -- the distinct sets of colours that segments have\n"
			"     and the segments that have each.  Per class, numbered in the order gfa1 first prints a segment of each: the name of its\n"
			"     first segment, its segments, bases, edges ((k+1)-mers), occurrences, number of colours and presence bits of --colors;\n"
			"     in front the colours and the classes, segments and edges by number of colours.  Needs -k and -s.  With --gpu the\n"
			"     classes are found on the device.  Goes with what --colors goes with, and with --colors, of the same colours (one walk\n"
			"     for all; this table is written last); not with --links, --bubbles or --text.\n\n"
			"   --classes-out <file name>\n     with --classes: write the table there instead of to the standard output\n\n"
			"   --classes-members <file name>\n     with --classes: also write the class of every segment there, one line per segment\n\n"
			"   --tracks <file|sequence>\n     instead of -f: the presence tracks of the input sequences as TSV of integers -- for every stretch of every sequence\n"
			"     the colours of --colors that share it.  Neighbouring segment occurrences of equal presence are one interval: sequence\n"
			"     (0-based), begin and end (the (k+1)-mers that start in [begin, end); in bases [begin, end + k)), occurrences, number of\n"
			"     colours and presence bits; in front the colours, the sequences, per colour its intervals, edges and the edges all\n"
			"     colours (core) or only this one (private) hold, and the intervals and edges by number of colours.  Needs -k and -s.\n"
			"     With --gpu the intervals are found on the device.  Goes with what --classes goes with, and with --classes, of the same\n"
			"     colours (one walk for all; this table is written last); not with --links, --bubbles or --text.\n\n"
			"   --tracks-of <integer>\n     with --tracks: the intervals of the sequences of this one colour only (default: all colours)\n\n"
			"   --tracks-out <file name>\n     with --tracks: write the table there instead of to the standard output\n\n"
			"   --tracks-bedgraph <file name>\n     with --tracks: also write the number of colours per interval there as bedGraph\n\n"
			"   --variants <file|sequence>\n     instead of -f: the alleles the genomes walk through the superbubbles as TSV of integers -- every sequence is walked\n"
			"     through every superbubble (of at most --superbubbles-max sides inside) on both strands; the walks from entrance to exit\n"
			"     that read the same inside sides are one allele.  Per allele: site (the row of --superbubbles), entrance and exit, its\n"
			"     number within the site, traversals, sides, edges, number of colours and presence bits, the span of its first traversal\n"
			"     (sequence, begin, end in bases, strand) and whether it is the reference's; in front the colours, the sequences and the\n"
			"     sites by number of alleles.  Needs -k and -s.  With --gpu the walks and the alleles are found on the device.  Goes with\n"
			"     what --tracks goes with, and with --tracks, of the same colours (this table is written last); not with --links,\n"
			"     --bubbles or --text.\n\n"
			"   --variants-ref <integer>\n     with --variants: the reference colour (default: none)\n\n"
			"   --variants-out <file name>\n     with --variants: write the table there instead of to the standard output\n\n"
			"   --variants-vcf <file name>\n     with --variants and --variants-ref: also write VCF 4.2 there, positions on the reference colour's sequences, one\n"
			"     sample per colour; not normalised (bcftools norm does that)\n\n"
			"   <file name>\n     (required)  input file name\n\n"
			"   This utility converts the binary output of TwoPaCo to another format\n\n");
	}
}

int main(int argc, char * argv[])
{
	try
	{
		std::string binFile, format;
		std::vector<std::string> fasta;
		TableOptions tables;
		bool textSet = false, compact = false;
		bool prefix = false, haveK = false, haveFormat = false, haveFile = false, gpu = false, textOnDevice = false;
		int device = 0;
		size_t k = 25, threads = 16;
		bool positionalOnly = false;
		for (int i = 1; i < argc; i++)
		{
			const std::string a = argv[i];
			auto value = [&](const std::string & id) -> std::string
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
			else if (a == "--compact") compact = true;
			else if (ParseTableOption(a, value, "Argument: ", tables)) continue;
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

		// A table instead of -f.  The link table goes with no other, the bubble table not with the colour table, the class table with
		// what the colour table goes with, none but the colour, the class and the link table's own complaint with --compact; the complaints are looked for from the last table back, the link table's last.
		const unsigned linksBit = 1u << LINKS;
		const TableCliRules rules = {"Argument: ", {VARIANTS, TRACKS, CLASSES, LOCATE, ANCHORS, SUPERBUBBLES, COMPONENTS, DISTANCES, BUBBLES, COLORS, LINKS}, true, haveFormat, compact, textSet,
			{0, 1u << COLORS, 1u << COLORS | linksBit, linksBit, linksBit, linksBit, linksBit, linksBit, 1u << BUBBLES | linksBit, 1u << BUBBLES | linksBit, 1u << BUBBLES | linksBit},
			{false, false, true, true, true, true, true, true, false, false, false}, 1, false, 0};
		CheckTableOptions(tables, rules);
		const TableRequest & request = tables.request;
		if (compact && format != "gfa1") throw ArgError("The compact text is gfa1 with every link once: it needs -f gfa1", "(--compact)");
		if (compact && textOnDevice) throw ArgError("The compact text is formatted by the host: not with --text device", "(--compact)");
		if (!haveK) throw ArgError("Required argument missing: kvalue", " ");
		if (!haveFormat && !request.Any()) throw ArgError("Required argument missing: format", " ");
		if (!haveFile) throw ArgError("Required argument missing: infile", " ");
		if (textOnDevice && !gpu) throw ArgError("Value 'device' does not meet constraint: the text is rendered on the device only with --gpu", "Argument: (--text)");
		const bool needsSequences = request.Any() || format == "gfa1" || format == "gfa2" || format == "fasta";
		if (needsSequences && fasta.empty()) throw ArgError("Required argument missing\n", "Argument: seqfilename");

		DumpStats stats;
		std::unique_ptr<DeviceLibrary> lib;
		if (gpu && needsSequences) lib.reset(new DeviceLibrary(device));  // before the first byte of output: no device is an error
		stats.threads = lib ? threads : 1;
		const bool deviceText = lib && textOnDevice;
		stats.text = deviceText ? "device" : "host";
		Out out(!deviceText && !compact);  // --text device, --compact: the header lines wait until the table is known to be good
		if (request.Any() && lib)
		{
			std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
			InputSequences seq;
			LoadedSequences loaded;
			LoadSequences(fasta, prefix, threads, seq, loaded);
			stats.loadMs = MsSince(t0);
			DumpTablesOnDevice(*lib, binFile, fasta, k, threads, seq, loaded, request, stats);
		}
		else if (request.Any()) DumpTables(binFile, fasta, k, prefix, request);
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
			std::fprintf(stderr, "error: %s for arg %s\n", e.what(), e.arg.c_str());  // thrown after parsing, graphdump.cpp:669-693
		}
		else
		{
			std::fprintf(stderr, "PARSE ERROR: %s\n             %s\n\nBrief USAGE: \n   %s  [-k <integer>] [-s <string>] ... -f <seq|group|dot|gfa1|gfa2|fasta> [--prefix] [--] [--version] [-h] <file name>\n\n"
				"For complete USAGE and HELP type: \n   %s --help\n\n", e.arg.c_str(), e.what(), argv[0], argv[0]);
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
