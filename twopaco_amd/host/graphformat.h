// graphformat.h -- the text of the compacted graph (gfa1 / gfa2 / fasta, reference src/graphdump/graphdump.cpp:379-585), shared
// by `graphdump` (junctiondump.cpp) and `twopaco --graph` (vertexenumerator.cpp).  Two layers:
//   * the sinks: one call per segment occurrence (an EVENT: two consecutive junction records of one sequence) and one per end
//     of sequence, exactly what the serial walk of junctiondump.cpp feeds them;
//   * the parallel formatter: given the EVENT TABLE of a stream (include/twopaco_hip.h, the tpc_segments_* group: name[],
//     first[], begin[], end[] per event in file order and seq_event_begin[] per sequence) every output line depends only on
//     its own event and the one before it, so workers format contiguous chunks of events.  The table and the letters of the
//     input sequences are all it reads: it never sees the stream's bytes.
// No device dependency: the table may come from the device library or from anywhere else (libtwopaco_host.so:
// tpch_graph_format), and graphdump links this unit without linking the device library.
#ifndef _GRAPH_FORMAT_H_
#define _GRAPH_FORMAT_H_

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "dnachar.h"

namespace TwoPaCo
{
	namespace GraphFormat
	{
		// ---------------------------------------------------------------------------------------- output
		class Out
		{
		public:
			// toStdout = false: the text only collects in Text() (a chunk of the parallel formatter, the head of a graph file)
			explicit Out(bool toStdout = true) : toStdout_(toStdout) {}
			~Out() { if (toStdout_) Flush(); }
			std::string & Text() { return buf_; }
			Out & operator << (const std::string & s) { buf_ += s; return Check(); }
			Out & operator << (const char * s) { buf_ += s; return Check(); }
			Out & operator << (char c) { buf_ += c; return Check(); }
			Out & operator << (int64_t v) { buf_ += std::to_string(static_cast<long long>(v)); return Check(); }
			Out & operator << (uint64_t v) { buf_ += std::to_string(static_cast<unsigned long long>(v)); return Check(); }
			Out & operator << (uint32_t v) { buf_ += std::to_string(v); return Check(); }
			void Flush()
			{
				if (!toStdout_) return;
				if (!buf_.empty()) std::fwrite(buf_.data(), 1, buf_.size(), stdout);
				buf_.clear();
				std::fflush(stdout);
			}

		private:
			Out & Check()
			{
				if (toStdout_ && buf_.size() > (1u << 20))
				{
					std::fwrite(buf_.data(), 1, buf_.size(), stdout);
					buf_.clear();
				}

				return *this;
			}

			bool toStdout_;
			std::string buf_;
		};

		inline int64_t Magnitude(int64_t x) { return x < 0 ? -x : x; }
		inline char Strand(int64_t x) { return x >= 0 ? '+' : '-'; }

		// ---------------------------------------------------------------------------------------- input sequences
		struct InputSequences
		{
			std::vector<std::string> name;
			std::vector<uint64_t> length;
			std::map<std::string, std::string> file;
			std::vector<uint32_t> fileIndex;   // per sequence: the index of its file among the files given (the colour table's by=file)
		};

		// What the serial walk reads record by record -- names, lengths, the letters as the parser upper-cases them -- read
		// once, files in parallel; and per sequence the positions of the valid letters other than A C G T N, which the packed
		// text holds as 'N' while the namer does not (SegmentNamer::Name: MakeUpChar of such a letter is -1).
		struct LoadedSequences
		{
			std::vector<std::string> body;
			std::vector<std::vector<uint64_t> > ambiguous;
		};

		template<class Fn> void RunParallel(size_t items, size_t threads, const Fn & fn)
		{
			std::atomic<size_t> cursor(0);
			auto work = [&]() { for (size_t i = cursor++; i < items; i = cursor++) fn(i); };
			std::vector<std::thread> pool;
			for (size_t t = 1; t < std::min(threads, items); t++) pool.emplace_back(work);
			work();
			for (std::thread & th : pool) th.join();
		}

		// throws std::runtime_error with the parser's text (the first error in file order)
		void LoadSequences(const std::vector<std::string> & fasta, bool prefixed, size_t threads, InputSequences & seq, LoadedSequences & loaded);

		// ---------------------------------------------------------------------------------------- sinks
		struct SegmentEvent
		{
			int64_t id;            // signed name
			uint64_t size;
			bool first;            // first sight of |id|
			uint64_t begin, end;   // junction positions in the sequence
			size_t sequence;
		};

		class SegmentSink
		{
		public:
			virtual ~SegmentSink() {}
			virtual void Segment(const SegmentEvent & e, const std::string & chr, size_t k) = 0;
			virtual void EndOfSequence(size_t sequence) = 0;
		};

		inline std::string SegmentBody(const SegmentEvent & e, const std::string & chr, size_t k)
		{
			const std::string body = chr.substr(e.begin, e.end + k - e.begin);
			return e.id > 0 ? body : DnaChar::ReverseCompliment(body);
		}

		class GfaSink : public SegmentSink
		{
		public:
			GfaSink(Out & out, const InputSequences & seq) : out_(out), seq_(seq), prevId_(0), prevSize_(0) {}

			void Segment(const SegmentEvent & e, const std::string & chr, size_t k)
			{
				if (e.first) SegmentLine(e, SegmentBody(e, chr, k));
				Occurrence(e, k);
				if (prevId_ != 0) Link(prevId_, prevSize_, e.id, e.size, k);
				prevId_ = e.id;
				prevSize_ = e.size;
				path_.push_back(e.id);
			}

			void EndOfSequence(size_t sequence)
			{
				if (!path_.empty()) Path(seq_.name[sequence]);
				path_.clear();
				prevId_ = 0;
			}

			// The parallel formatter enters a sequence in the middle (Resume: the event before the chunk's first one, 0 when that
			// begins its sequence) and hands the whole path to the worker that holds the sequence's last event.
			void Resume(int64_t prevId, uint64_t prevSize)
			{
				path_.clear();
				prevId_ = prevId;
				prevSize_ = prevSize;
			}

			void EndOfSequence(size_t sequence, const int64_t * name, size_t count)
			{
				path_.assign(name, name + count);
				EndOfSequence(sequence);
			}

		protected:
			virtual void SegmentLine(const SegmentEvent & e, const std::string & body) = 0;
			virtual void Occurrence(const SegmentEvent & e, size_t k) = 0;
			virtual void Link(int64_t a, uint64_t aSize, int64_t b, uint64_t bSize, size_t k) = 0;
			virtual void Path(const std::string & name) = 0;
			Out & out_;
			const InputSequences & seq_;
			std::vector<int64_t> path_;

		private:
			int64_t prevId_;
			uint64_t prevSize_;
		};

		class Gfa1Sink : public GfaSink
		{
		public:
			Gfa1Sink(Out & out, const InputSequences & seq) : GfaSink(out, seq) {}

		protected:
			void SegmentLine(const SegmentEvent & e, const std::string & body) { out_ << "S\t" << Magnitude(e.id) << '\t' << body << '\n'; }

			void Occurrence(const SegmentEvent & e, size_t)
			{
				out_ << "C\t" << Magnitude(e.id) << '\t' << Strand(e.id) << '\t' << seq_.name[e.sequence] << "\t+\t" << e.end << '\n';
			}

			void Link(int64_t a, uint64_t, int64_t b, uint64_t, size_t k)
			{
				out_ << "L\t" << Magnitude(a) << '\t' << Strand(a) << '\t' << Magnitude(b) << '\t' << Strand(b) << '\t' << uint64_t(k) << "M\n";
			}

			void Path(const std::string & name)
			{
				out_ << "P\t" << name << '\t';
				for (size_t i = 0; i < path_.size(); i++) out_ << Magnitude(path_[i]) << Strand(path_[i]) << (i + 1 < path_.size() ? "," : "\t*\n");
			}
		};

		// The COMPACT gfa1: the gfa1 text without its C lines and with every link once -- the L line of an event is printed only
		// when the event closes the first occurrence of its link (the link_first bits of include/twopaco_hip.h's link table; the
		// caller announces the bit of an event with NextLink before it hands the event to Segment).  S lines with a body and P
		// lines are what Gfa1Sink prints.
		class CompactGfa1Sink : public Gfa1Sink
		{
		public:
			CompactGfa1Sink(Out & out, const InputSequences & seq) : Gfa1Sink(out, seq), printLink_(false) {}
			void NextLink(bool first) { printLink_ = first; }

		protected:
			void Occurrence(const SegmentEvent &, size_t) {}

			void Link(int64_t a, uint64_t aSize, int64_t b, uint64_t bSize, size_t k)
			{
				if (printLink_) Gfa1Sink::Link(a, aSize, b, bSize, k);
			}

		private:
			bool printLink_;
		};

		class Gfa2Sink : public GfaSink
		{
		public:
			Gfa2Sink(Out & out, const InputSequences & seq) : GfaSink(out, seq) {}

		protected:
			static std::string At(uint64_t pos, uint64_t length) { return pos == length ? std::to_string(pos) + "$" : std::to_string(pos); }

			void SegmentLine(const SegmentEvent & e, const std::string & body) { out_ << "S\t" << Magnitude(e.id) << '\t' << e.size << '\t' << body << '\n'; }

			void Occurrence(const SegmentEvent & e, size_t k)
			{
				const uint64_t total = seq_.length[e.sequence];
				out_ << "F\t" << Magnitude(e.id) << '\t' << seq_.name[e.sequence] << Strand(e.id) << "\t0\t" << e.size << "$\t" << At(e.begin, total) << '\t'
					<< At(e.end + k, total) << '\t' << uint64_t(k) << "M\n";
			}

			void Link(int64_t a, uint64_t aSize, int64_t b, uint64_t bSize, size_t k)
			{
				const uint64_t a0 = a > 0 ? aSize - k : 0, a1 = a > 0 ? aSize : k;   // the overlapping k-mer on each segment
				const uint64_t b0 = b > 0 ? 0 : bSize - k, b1 = b > 0 ? k : bSize;
				out_ << "E\t" << Magnitude(a) << Strand(a) << '\t' << Magnitude(b) << Strand(b) << '\t' << At(a0, aSize) << '\t' << At(a1, aSize) << '\t'
					<< At(b0, bSize) << '\t' << At(b1, bSize) << '\t' << uint64_t(k) << "M\n";
			}

			void Path(const std::string & name)
			{
				out_ << "O\t" << name << "p\t";
				for (size_t i = 0; i < path_.size(); i++) out_ << Magnitude(path_[i]) << Strand(path_[i]) << (i + 1 < path_.size() ? " " : "\n");
			}
		};

		class FastaSink : public SegmentSink
		{
		public:
			explicit FastaSink(Out & out) : out_(out) {}

			void Segment(const SegmentEvent & e, const std::string & chr, size_t k)
			{
				if (!e.first) return;
				out_ << '>' << Magnitude(e.id) << '\n';
				const std::string body = SegmentBody(e, chr, k);
				for (size_t i = 0; i < body.size(); i += 80) out_ << body.substr(i, 80) << '\n';
			}

			void EndOfSequence(size_t) {}

		private:
			Out & out_;
		};

		// ---------------------------------------------------------------------------------------- the parallel formatter
		// The event table of a stream, as include/twopaco_hip.h defines it (arrays of the caller, host memory).
		struct EventTable
		{
			uint64_t events;
			const int64_t * name;            // [events]
			const uint32_t * first;          // [(events + 31) / 32] bit e % 32 of word e / 32
			const uint32_t * begin;          // [events]
			const uint32_t * end;            // [events]
			uint64_t sequences;
			const uint32_t * seqEventBegin;  // [sequences + 1]
			const uint32_t * linkFirst;      // optional, laid out as first: the link table's first bits.  Given, gfa1 is formatted COMPACT
			EventTable() : events(0), name(0), first(0), begin(0), end(0), sequences(0), seqEventBegin(0), linkFirst(0) {}
		};

		bool IsGraphFormat(const std::string & format);  // gfa1, gfa2, fasta

		// The lines in front of the first segment, as graphdump prints them: "H\tVN:Z:..." and, for gfa1, one S line per input
		// sequence whose UR:Z: tag is the file's name as it was given.
		// compact (gfa1 only): the H line alone.
		void HeaderLines(const std::string & format, const InputSequences & seq, Out & out, bool compact = false);

		// Everything the formatter indexes with is checked here (the table may come from anywhere): the sequences' event ranges
		// ascend from 0 to the event count, there are as many sequences as the FASTA files hold, every event lies inside its
		// sequence.  Throws std::runtime_error.
		void CheckEventTable(const EventTable & table, const LoadedSequences & loaded, size_t k, size_t threads);

		// The text of all events, formatted by `threads` workers in contiguous chunks.  fd < 0: to stdout, in order, written by
		// the calling thread.  Otherwise to the regular file open on fd, starting at fileOffset: every worker writes its own
		// chunk with pwrite at the sum of the earlier chunks' sizes, into space preallocated with posix_fallocate; returns the
		// bytes written (the caller truncates the file to fileOffset + that).  The table must have passed CheckEventTable.
		uint64_t FormatEvents(const EventTable & table, const InputSequences & seq, const LoadedSequences & loaded, size_t k, const std::string & format,
			size_t threads, int fd, uint64_t fileOffset);

		// The file outPath (created or truncated; removed again when anything fails): the header lines, then what `events` writes
		// from the offset it is given on (it returns its bytes); the file is truncated to the sum.
		void WriteGraphFileWith(const std::string & format, const InputSequences & seq, const std::string & outPath,
			const std::function<uint64_t(int fd, uint64_t fileOffset)> & events, bool compact = false);

		// What the device formatter (include/twopaco_hip.h: tpc_segments_text_plan) takes beside the event table: the names as they
		// are printed, as one blob with offsets, and the letter at every ambiguous position in the order of the positions.
		struct DeviceTextInput
		{
			std::string names;
			std::vector<uint64_t> nameOffset;   // [sequences + 1]
			std::vector<uint8_t> ambiguousLetter;
		};

		inline void MakeDeviceTextInput(const InputSequences & seq, const LoadedSequences & loaded, DeviceTextInput & out)
		{
			out.nameOffset.assign(1, 0);
			for (const std::string & name : seq.name)
			{
				out.names += name;
				out.nameOffset.push_back(out.names.size());
			}

			for (size_t r = 0; r < loaded.body.size(); r++)
			{
				for (uint64_t at : loaded.ambiguous[r]) out.ambiguousLetter.push_back(uint8_t(loaded.body[r][at]));
			}
		}

		// TPC_TEXT_GFA1 / _GFA2 / _FASTA of include/twopaco_hip.h
		inline int DeviceTextFormat(const std::string & format) { return format == "gfa1" ? 1 : format == "gfa2" ? 2 : format == "fasta" ? 3 : 0; }

		// ---------------------------------------------------------------------------------------- the segment colour table
		// Which colours hold each segment, how often, on which strand (include/twopaco_hip.h, the tpc_segments_colors_* group, defines
		// rows, columns and the histogram).  The arrays come from ComputeColors below -- the serial statement of the table -- or from
		// the device (csrc/tpc_colors.hip); WriteColors prints either as the same bytes.
		struct ColorTable
		{
			uint64_t colors;
			std::vector<uint32_t> firstEvent, occurrences, forward, nColors;   // [rows]
			std::vector<uint32_t> presence;                                    // [rows][Words()], bit c % 32 of word c / 32
			std::vector<uint64_t> histSegments, histBases;                     // [colors + 1]
			ColorTable() : colors(0) {}
			size_t Rows() const { return firstEvent.size(); }
			size_t Words() const { return size_t((colors + 31) / 32); }
		};

		// The colour of every sequence and the label of every colour: one colour per file (label: the file name as given) or one
		// per sequence (label: the 1-based sequence number, a tab, its file name).
		struct ColorMap
		{
			bool bySequence;
			std::vector<uint32_t> colorOfSequence;
			std::vector<std::string> label;
			ColorMap() : bySequence(false) {}
		};

		void MakeColorMap(const InputSequences & seq, const std::vector<std::string> & fasta, bool bySequence, ColorMap & out);

		// One pass over the events with a hash map from |name| to its row.  The table must be one whose walk did not fail; every
		// event's sequence needs a colour below `colors` (std::runtime_error otherwise).
		void ComputeColors(const EventTable & table, size_t k, const std::vector<uint32_t> & colorOfSequence, uint64_t colors, ColorTable & out);

		// The TSV text: "#twopaco-colors" header, one "#color" line per colour, one line per row (name, length, occurrences, forward,
		// n_colors, presence as ceil(colors / 4) hex digits, digit j from the left = colours 4j .. 4j + 3, colour 4j + b = 1 << b),
		// "#hist" lines of the non-empty bins.  To stdout (path empty) or into the file `path` (removed again when writing fails).
		void WriteColors(const EventTable & table, size_t k, const ColorMap & map, const ColorTable & colors, const std::string & path);

		// ---------------------------------------------------------------------------------------- the link table
		// Every distinct link of the graph once (include/twopaco_hip.h, the tpc_segments_links_* group, defines occurrence, class,
		// rows and first bits).  The arrays come from ComputeLinks below -- the serial statement -- or from the device
		// (csrc/tpc_links.hip); WriteLinks prints either as the same bytes.
		struct LinkTable
		{
			uint64_t occurrences;
			std::vector<uint32_t> firstEvent, count, same;   // [rows]
			std::vector<uint32_t> linkFirst;                 // [(events + 31) / 32]
			LinkTable() : occurrences(0) {}
			size_t Rows() const { return firstEvent.size(); }
		};

		// One pass over the events with a hash map from the class -- the smaller of (a, b) and (-b, -a) -- to its row.  The table
		// must be one whose walk did not fail.
		void ComputeLinks(const EventTable & table, LinkTable & out);

		// The TSV text: "#twopaco-links\t1\tk=<k>\tsegments=<S>\tlinks=<N>\toccurrences=<M>", then one line per row as it is spelled:
		// |from|, its strand, |to|, its strand, count, same.  To stdout (path empty) or into the file `path` (removed again when
		// writing fails).
		void WriteLinks(const EventTable & table, size_t k, uint64_t segments, const LinkTable & links, const std::string & path);

		// ---------------------------------------------------------------------------------------- the simple bubbles
		// Where the genomes differ: two segments leave one side of a segment, touch nothing else and meet again at one side of
		// another (include/twopaco_hip.h, the tpc_segments_bubbles_* group, defines side, arc, degree, bubble, canonical orientation
		// and the orders; simple bubbles only -- three alleles at one place, nested bubbles and superbubbles are in the superbubble
		// table below).  The
		// arrays come from ComputeBubbles below -- the serial statement -- or from the device (csrc/tpc_bubbles.hip); WriteBubbles
		// prints either as the same bytes.  A side is row * 2 + (1 when the strand is '-'), the rows being the colour table's.
		struct BubbleTable
		{
			uint64_t sides, arcs;
			std::vector<uint32_t> source, armA, armB, sink;   // [bubbles], side codes
			uint64_t hist[6];                                 // sides of degree 0, 1, 2, 3, 4, 5 or more
			BubbleTable() : sides(0), arcs(0), hist{0, 0, 0, 0, 0, 0} {}
			size_t Rows() const { return source.size(); }
		};

		// The definition stated with std:: containers: the row of every segment by a hash map from |name|, the arcs of every link
		// row into one std::set of heads per side, then every side against the definition.  The table must be one whose walk did
		// not fail, `links` its link rows.
		void ComputeBubbles(const EventTable & table, const LinkTable & links, BubbleTable & out);

		// The TSV text: "#twopaco-bubbles\t1\tby=<file|sequence>\tk=<k>\tcolors=<C>\tsegments=<S>\tlinks=<N>\tbubbles=<B>", the colour
		// table's "#color" lines, "#sides\t<degree>\t<count>" for the bins 0, 1, 2, 3, 4, 5+ that hold sides (0: the dead ends), then
		// one line per bubble: source, arm_a, arm_b, sink each as |name| and strand, then of the two arms the lengths, occurrences,
		// numbers of colours and presence hex of their colour rows, and the number of colours that hold both arms.  `colors` is the
		// colour table of the same event table (its rows are the sides' rows).  To stdout (path empty) or into the file `path`
		// (removed again when writing fails).
		void WriteBubbles(const EventTable & table, size_t k, const ColorMap & map, const ColorTable & colors, uint64_t links, const BubbleTable & bubbles,
			const std::string & path);

		// ---------------------------------------------------------------------------------------- the genome distance matrices
		// How much every colour shares with every other one (include/twopaco_hip.h, the tpc_segments_distances_* group, defines
		// weight, rows and the two matrices; edges -- (k+1)-mers -- not bases, and whatever the colour table calls a row counts).
		// The arrays come from ComputeDistances below -- the serial statement -- or from the device (csrc/tpc_distances.hip);
		// WriteDistances and WriteDistancesPhylip print either as the same bytes.
		struct DistanceTable
		{
			uint64_t colors;
			std::vector<uint64_t> segments, edges;   // [colors][colors], row-major, symmetric, stored in full
			DistanceTable() : colors(0) {}
		};

		// Two nested loops over the set bits of every row of the colour table; weight = end - begin of the row's first event.
		void ComputeDistances(const EventTable & table, const ColorTable & colors, DistanceTable & out);

		// The TSV text: "#twopaco-distances\t1\tby=<file|sequence>\tk=<k>\tcolors=<C>\tsegments=<S>", the colour table's "#color" lines,
		// "#self\t<c>\t<segments[c][c]>\t<edges[c][c]>" per colour, then "<i>\t<j>\t<segments[i][j]>\t<edges[i][j]>" for every i < j, i
		// ascending then j, the pairs that share nothing included.  Integers only: a reader gets the Jaccard similarity as
		// e_ij / (e_ii + e_jj - e_ij).  To stdout (path empty) or into the file `path` (removed again when writing fails).
		void WriteDistances(size_t k, const ColorMap & map, uint64_t rows, const DistanceTable & distances, const std::string & path);

		// The relaxed PHYLIP square matrix neighbour-joining tools read, into the file `path`: the line "C", then per colour its
		// label with every byte <= ' ' replaced by '_' and C values, each preceded by one space and printed with %.6f:
		// d = (u - e_ij) / u with u = e_ii + e_jj - e_ij, the Jaccard distance over edges; 0 when u == 0 and on the diagonal.  One
		// correctly rounded division of two exactly represented integers.
		void WriteDistancesPhylip(const ColorMap & map, const DistanceTable & distances, const std::string & path);

		// Both files of the distance table, or neither: the PHYLIP matrix first when phylipPath is given, then the TSV (to stdout when
		// path is empty); when the TSV cannot be written the PHYLIP file is removed again before the error is thrown.
		void WriteDistanceFiles(size_t k, const ColorMap & map, uint64_t rows, const DistanceTable & distances, const std::string & path, const std::string & phylipPath);

		// ---------------------------------------------------------------------------------------- the connected components
		// Which pieces of the graph hang together (include/twopaco_hip.h, the tpc_segments_components_* group, states the definition
		// in the same words).  ROW: a segment, the rows are the colour table's.  JOINED: the rows of `from` and `to` of a link row
		// are joined; strands do not matter, a self-loop and a link that is its own reverse join a row to itself, 'N'-named segments
		// are segments like any other.  COMPONENT: a class of the transitive closure of JOINED; a segment that no link touches is a
		// component of one; its ROOT is its smallest row.  COMPONENT ID: components are numbered from 0, ascending by root, the
		// order in which gfa1 first prints a segment of each.  Per component: root, segments, links (the link rows whose ends lie in
		// it; every link row lies in exactly one), length (the sum of its segments' lengths in bases), edges (the sum of their
		// weights, end - begin of the row's first event: length - k per segment), occurrences (the sum of the colour rows'
		// occurrences), presence (the OR of the colour rows' presence words) and n_colors, its popcount.  The sums are 64-bit.
		// Every input sequence with an event lies in exactly one component, because consecutive segments of a sequence are linked:
		// with one colour per sequence, presence says which contigs make up a component.  The segments of all components sum to
		// the rows, their links to the link rows.  The arrays come from ComputeComponents below -- the serial statement -- or from
		// the device (csrc/tpc_components.hip); WriteComponents and WriteComponentMembers print either as the same bytes.
		struct ComponentTable
		{
			std::vector<uint32_t> component;                                   // [rows]
			std::vector<uint32_t> root;                                        // [components]
			std::vector<uint64_t> segments, links, length, edges, occurrences; // [components]
			std::vector<uint32_t> presence;                                    // [components][colors.Words()]
			size_t Rows() const { return root.size(); }
			uint64_t Largest() const { return segments.empty() ? 0 : *std::max_element(segments.begin(), segments.end()); }
		};

		// The definition stated with std:: containers: the row of every segment by a hash map from |name|, a plain union-find over
		// the link rows, the ids by one pass over the rows, then the sums.  The table must be one whose walk did not fail, `links`
		// its link rows and `colors` its colour table.
		void ComputeComponents(const EventTable & table, size_t k, const LinkTable & links, const ColorTable & colors, ComponentTable & out);

		// The TSV text: "#twopaco-components\t1\tby=<file|sequence>\tk=<k>\tcolors=<C>\tsegments=<S>\tlinks=<N>\tcomponents=<P>", the
		// colour table's "#color" lines, "#size\t<b>\t<components>\t<segments>" for every b = floor(log2(segments[p])) that occurs,
		// ascending, then one line per component: id, the name of the root segment, segments, links, length, edges, occurrences,
		// n_colors and presence as hex (as the colour table prints it).  To stdout (path empty) or into the file `path` (removed again
		// when writing fails).
		void WriteComponents(const EventTable & table, size_t k, const ColorMap & map, const ColorTable & colors, uint64_t links, const ComponentTable & components,
			const std::string & path);

		// The members: "#twopaco-component-members\t1\tk=<k>\tsegments=<S>\tcomponents=<P>", then "<name>\t<id>" per row in row order,
		// into the file `path`.
		void WriteComponentMembers(const EventTable & table, size_t k, const ColorTable & colors, const ComponentTable & components, const std::string & path);

		// Both files of the component table, or neither: the members first when membersPath is given, then the TSV (to stdout when
		// path is empty); when the TSV cannot be written the members file is removed again before the error is thrown.
		void WriteComponentFiles(const EventTable & table, size_t k, const ColorMap & map, const ColorTable & colors, uint64_t links, const ComponentTable & components,
			const std::string & path, const std::string & membersPath);

		// ---------------------------------------------------------------------------------------- the colour classes
		// Which segments share their set of genomes (include/twopaco_hip.h, the tpc_segments_classes_* group, states the definition
		// in the same words).  ROW: a row of the colour table, 'N'-named segments included.  CLASS: the rows whose presence words are
		// all equal; its FIRST is its smallest row.  CLASS ID: classes are numbered from 0, ascending by first, the order in which
		// gfa1 first prints a segment of each.  Per class: first, segments, length (the sum of the segments' lengths in bases), edges
		// (the sum of end - begin of each row's first event, the weight of the distance matrices), occurrences (the sum of the colour
		// rows' occurrences), presence (the words every row of the class holds) and n_colors, its popcount.  The sums are 64-bit.
		// The segments of all classes sum to the rows, those of the classes of n colours to the colour table's "#hist n", and the
		// distance matrices are the sums of segments and edges over the classes that hold both colours.  The arrays come from
		// ComputeClasses below -- the serial statement -- or from the device (csrc/tpc_classes.hip); WriteClasses and
		// WriteClassMembers print either as the same bytes.
		struct ClassTable
		{
			std::vector<uint32_t> classOf;                                     // [rows]
			std::vector<uint32_t> first;                                       // [classes]
			std::vector<uint64_t> segments, length, edges, occurrences;        // [classes]
			std::vector<uint32_t> presence;                                    // [classes][colors.Words()]
			size_t Rows() const { return first.size(); }
			uint64_t Largest() const { return segments.empty() ? 0 : *std::max_element(segments.begin(), segments.end()); }
		};

		// The definition stated with std:: containers: an ordered map from the presence words of a row to its class, filled in row
		// order, so that the ids ascend by first; then the sums.  `colors` is the colour table of `table`.
		void ComputeClasses(const EventTable & table, size_t k, const ColorTable & colors, ClassTable & out);

		// The TSV text: "#twopaco-classes\t1\tby=<file|sequence>\tk=<k>\tcolors=<C>\tsegments=<S>\tclasses=<P>", the colour table's
		// "#color" lines, "#sets\t<n>\t<classes>\t<segments>\t<edges>" for every number of colours n that a class has, ascending, then
		// one line per class: id, the name of the first segment, segments, length, edges, occurrences, n_colors and presence as hex (as
		// the colour table prints it).  To stdout (path empty) or into the file `path` (removed again when writing fails).
		void WriteClasses(const EventTable & table, size_t k, const ColorMap & map, const ColorTable & colors, const ClassTable & classes, const std::string & path);

		// The members: "#twopaco-class-members\t1\tk=<k>\tsegments=<S>\tclasses=<P>", then "<name>\t<id>" per row in row order, into
		// the file `path`.
		void WriteClassMembers(const EventTable & table, size_t k, const ColorTable & colors, const ClassTable & classes, const std::string & path);

		// Both files of the class table, or neither: the members first when membersPath is given, then the TSV (to stdout when path
		// is empty); when the TSV cannot be written the members file is removed again before the error is thrown.
		void WriteClassFiles(const EventTable & table, size_t k, const ColorMap & map, const ColorTable & colors, const ClassTable & classes, const std::string & path,
			const std::string & membersPath);

		// ---------------------------------------------------------------------------------------- the presence tracks
		// Which colours share each stretch of every sequence (include/twopaco_hip.h, the tpc_segments_tracks_* group, states the
		// definition in the same words).  row(e), seq(e) and colour(e) = colorOfSequence[seq(e)] are those of the colour table.  With
		// only == ALL every event is SELECTED, otherwise those with colour(e) == only.  A selected event e CONTINUES e - 1 when both lie
		// in one sequence and the presence words of their rows are all equal.  An INTERVAL is a maximal run firstEvent .. lastEvent of
		// selected events each continuing the one before; it stands for the (k+1)-mers that start at [begin[first], end[last]) of its
		// sequence, in bases [begin[first], end[last] + k); its presence and n_colors are those of row(first).  Intervals ascend by
		// firstEvent and tile every sequence's events.  Per colour: intervals, edges (end[last] - begin[first] summed), coreEdges
		// (n_colors == C) and privateEdges (n_colors == 1); per depth n = 0 .. C: depthIntervals and depthEdges.  The arrays come from
		// ComputeTracks below -- the serial statement -- or from the device (csrc/tpc_tracks.hip); the writers print either as the same
		// bytes.
		struct TrackTable
		{
			static const uint32_t ALL = 0xFFFFFFFFu;                           // only: every colour
			uint64_t colors, segments;
			uint32_t only;
			std::vector<uint32_t> firstEvent, lastEvent, row;                  // [intervals]
			std::vector<uint64_t> intervals, edges, coreEdges, privateEdges;   // [colors]
			std::vector<uint64_t> depthIntervals, depthEdges;                  // [colors + 1]
			TrackTable() : colors(0), segments(0), only(ALL) {}
			size_t Rows() const { return firstEvent.size(); }
		};

		// The definition as a plain loop over the events: the row of every event by a hash map from |name|, as ComputeColors numbers
		// them.  `colors` is the colour table of `table` under colorOfSequence.  The table must be one whose walk did not fail; every
		// sequence needs a colour below nColors, and only < nColors or ALL (std::runtime_error otherwise).  No device dependency.
		void ComputeTracks(const EventTable & table, size_t k, const std::vector<uint32_t> & colorOfSequence, uint64_t nColors, const ColorTable & colors, uint32_t only,
			TrackTable & out);

		// The TSV text: "#twopaco-tracks\t1\tby=<file|sequence>\tk=<k>\tcolors=<C>\tsegments=<S>\tof=<c|all>\tintervals=<I>", the colour
		// table's "#color" lines, the anchor table's "#sequence" lines, "#genome\t<c>\t<intervals>\t<edges>\t<core_edges>\t
		// <private_edges>" for every selected colour, zeros included, "#depth\t<n>\t<intervals>\t<edges>" for every n that occurs, then
		// one line per interval: sequence (0-based), begin, end ((k+1)-mer starts, half-open), events, n_colors and presence as hex (as
		// the colour table prints it).  To stdout (path empty) or into the file `path` (removed again when writing fails).
		void WriteTracks(const EventTable & table, size_t k, const ColorMap & map, const InputSequences & seq, const ColorTable & colors, const TrackTable & tracks,
			const std::string & path);

		// bedGraph into the file `path`: the track line, then "<name>\t<begin>\t<end>\t<n_colors>" per interval in the table's order,
		// not merged further; sequences are named as the anchor PAF names them.
		void WriteTracksBedGraph(const EventTable & table, size_t k, const ColorMap & map, const InputSequences & seq, const ColorTable & colors, const TrackTable & tracks,
			const std::string & path);

		// Both files, or neither: the bedGraph first when bedGraphPath is given, then the TSV (to stdout when path is empty); when the
		// TSV cannot be written the bedGraph file is removed again before the error is thrown.
		void WriteTrackFiles(const EventTable & table, size_t k, const ColorMap & map, const InputSequences & seq, const ColorTable & colors, const TrackTable & tracks,
			const std::string & path, const std::string & bedGraphPath);

		// ---------------------------------------------------------------------------------------- the superbubbles
		// Where the genomes differ, beyond two alleles (include/twopaco_hip.h, the tpc_segments_superbubbles_* group, states the
		// definition in the same words; Onodera, Sadakane and Shibuya 2013).  Rows, sides (code = row * 2 + minus, rev(code) = code ^ 1),
		// arcs, out(u) and deg(u) are those of the simple bubbles; in(v) = { rev(w) : w in out(rev(v)) }.  For sides s != t, U(s, t) is
		// the set of sides reachable from s along arcs without leaving t (s and t included; a path may end at t but not continue
		// through it).  (s, t) is a SUPERBUBBLE with entrance s, exit t and inside U \ {s, t} when: 1. deg(s) >= 2 and t is in U;
		// 2. MATCHING: U equals the set of sides from which t is reachable along arcs without entering s (where 3 holds: every side of
		// U other than t has all its out-neighbours in U and at least one, every side of U other than s has all its in-neighbours in
		// U); 3. ACYCLIC: the arcs with both ends in U form no cycle, which includes no arc t -> s and no self-loop; 4. ONE STRAND PER
		// SEGMENT: no two sides of U have the same row; 5. MINIMAL: no side t' of the inside makes (s, t') satisfy 1-4; 6. BOUNDED:
		// |inside| <= maxInside, 2 .. 62, so a superbubble is at most 64 sides.  A side is the entrance of at most one superbubble,
		// exit(s).  (s, t) is REPORTED when exit(s) = t and either code(s) < code(rev(t)) or exit(rev(t)) != rev(s); rows ascend by
		// entrance code.  Per row: entrance, exit, inside (the number of sides inside), arcs (both ends in U), paths (the distinct arc
		// paths from s to t), minEdges and maxEdges (the smallest and largest sum over an s-t path of the weights, length - k, of its
		// inside segments), presence (the OR of the inside rows' colour words), nColors, and the members: the inside sides ascending.
		// The arrays come from ComputeSuperbubbles below -- the serial statement -- or from the device (csrc/tpc_superbubbles.hip);
		// the writers print either as the same bytes.
		struct SuperbubbleTable
		{
			uint64_t sides, arcs, unmirrored;                        // arcs of the whole graph; entrances whose mirror is missing
			uint32_t maxInside;
			std::vector<uint32_t> entrance, exit, inside, arcsIn, nColors;   // [superbubbles]
			std::vector<uint64_t> paths, minEdges, maxEdges;                   // [superbubbles]
			std::vector<uint32_t> presence;                                    // [superbubbles][colors.Words()]
			std::vector<uint32_t> memberOffset, members;                       // [superbubbles + 1], [members]: side codes
			SuperbubbleTable() : sides(0), arcs(0), unmirrored(0), maxInside(62) {}
			size_t Rows() const { return entrance.size(); }
		};

		// The definition's procedure stated with std:: containers: the arcs of every link row into one std::set of heads per side,
		// then per side of degree 2 or more Onodera's walk -- a list of the sides seen with their unvisited in-neighbours counted down,
		// failing on a dead end, an arc back to the entrance, the other strand of a listed side and an entry beyond maxInside + 2 --
		// the reporting rule, and per reported row the sums over the walk's own topological order.  No device dependency.
		void ComputeSuperbubbles(const EventTable & table, size_t k, const LinkTable & links, const ColorTable & colors, uint32_t maxInside, SuperbubbleTable & out);

		// The TSV text: "#twopaco-superbubbles\t1\tby=<file|sequence>\tk=<k>\tcolors=<C>\tsegments=<S>\tlinks=<N>\tmax_inside=<M>\t
		// superbubbles=<B>", the colour table's "#color" lines, "#inside\t<n>\t<count>" for every inside size that occurs, ascending,
		// then one line per row: entrance and exit each as |name| and strand, inside, arcs, paths, min_edges, max_edges, n_colors and
		// presence as hex.  To stdout (path empty) or into the file `path` (removed again when writing fails).
		void WriteSuperbubbles(const EventTable & table, size_t k, const ColorMap & map, const ColorTable & colors, uint64_t links, const SuperbubbleTable & superbubbles,
			const std::string & path);

		// The members: "#twopaco-superbubble-members\t1\tk=<k>\tsegments=<S>\tmax_inside=<M>\tsuperbubbles=<B>\tmembers=<T>", then
		// "<row of the table, from 0>\t<name>\t<strand>" per member, into the file `path`.
		void WriteSuperbubbleMembers(const EventTable & table, size_t k, const ColorTable & colors, const SuperbubbleTable & superbubbles, const std::string & path);

		// Both files, or neither: the members first when membersPath is given, then the TSV (to stdout when path is empty); when the
		// TSV cannot be written the members file is removed again before the error is thrown.
		void WriteSuperbubbleFiles(const EventTable & table, size_t k, const ColorMap & map, const ColorTable & colors, uint64_t links, const SuperbubbleTable & superbubbles,
			const std::string & path, const std::string & membersPath);

		// ---------------------------------------------------------------------------------------- the variants
		// Which allele every genome carries through every superbubble, what it spells and where it lies (include/twopaco_hip.h, the
		// tpc_segments_variants_* group, states the definition in the same words).  side(e) = row(e) * 2 + (name[e] < 0).  A WALK (e, d)
		// visits e, e + 1, .. reading side(x) (d = 0, '+') or e, e - 1, .. reading side(x) ^ 1 (d = 1, '-') and never leaves the events
		// of seq(e).  It is a TRAVERSAL of superbubble row b when its first side is entrance[b] and every following side is a member of
		// b until one is exit[b], at the event `last`, within maxInside + 1 steps.  A walk that reads a side that is neither counts in
		// `strays`.  Traversals are numbered by (e, d), '+' first; mask has bit i set when member i of the row was read; edges =
		// |begin[hi] - end[lo]| over lo, hi = the smaller and larger of start and last.  An ALLELE is the traversals of one row with one
		// mask, its `first` the smallest of them; alleles ascend by (row, first).  A SITE is a row with a traversal: alleleOffset[b] ..
		// alleleOffset[b + 1] are its alleles.  With a reference colour ref != NONE, refAllele[b] is the allele of the smallest
		// traversal of b that starts in a sequence of that colour (NONE without one), refTraversals[b] their number.  The arrays come
		// from ComputeVariants below -- the serial statement -- or from the device (csrc/tpc_variants.hip); the writers print either as
		// the same bytes.
		struct VariantTable
		{
			static const uint32_t NONE = 0xFFFFFFFFu;                          // ref: no reference; refAllele[]: no traversal of the reference
			uint64_t colors, segments, strays;
			uint32_t ref;
			std::vector<uint32_t> start, last, dir, row, edges;                // [traversals]
			std::vector<uint64_t> mask;                                        // [traversals]
			std::vector<uint32_t> alleleRow, sides, alleleEdges, first, nColors; // [alleles]
			std::vector<uint64_t> alleleMask, traversals;                      // [alleles]
			std::vector<uint32_t> presence;                                    // [alleles][colors.Words()]
			std::vector<uint32_t> alleleOffset;                                // [superbubbles + 1]
			std::vector<uint32_t> refAllele;                                   // [superbubbles]
			std::vector<uint64_t> siteTraversals, refTraversals;               // [superbubbles]
			VariantTable() : colors(0), segments(0), strays(0), ref(NONE) {}
			size_t Traversals() const { return start.size(); }
			size_t Alleles() const { return first.size(); }
			size_t Sites() const
			{
				size_t n = 0;
				for (size_t b = 0; b + 1 < alleleOffset.size(); b++) n += alleleOffset[b + 1] > alleleOffset[b] ? 1 : 0;
				return n;
			}
		};

		// The definition as plain loops: the side of every event by a hash map from |name|, as ComputeColors numbers the rows, a map
		// from entrance to row, both walks of every event, an ordered map from (row, mask) to the allele.  `colors` and `superbubbles`
		// are the tables of `table`.  Every sequence needs a colour below nColors, and ref < nColors or NONE (std::runtime_error
		// otherwise).  No device dependency.
		void ComputeVariants(const EventTable & table, size_t k, const std::vector<uint32_t> & colorOfSequence, uint64_t nColors, const ColorTable & colors,
			const SuperbubbleTable & superbubbles, uint32_t ref, VariantTable & out);

		// The TSV text: "#twopaco-variants\t1\tby=<file|sequence>\tk=<k>\tcolors=<C>\tsegments=<S>\tsuperbubbles=<B>\tmax_inside=<M>\t
		// ref=<R|none>\tsites=<..>\talleles=<..>\ttraversals=<..>", the colour table's "#color" lines, the anchor table's "#sequence"
		// lines, "#alleles\t<n>\t<sites>" for every number of alleles a site has, ascending, then one line per allele: site (the
		// superbubble row), entrance and exit each as |name| and strand, allele (from 0 within the site), traversals, sides, edges,
		// n_colors, presence as hex, then sequence (0-based), begin, end (bases, half-open) and strand of its first traversal, and
		// is_ref.  Integers and hex only.  To stdout (path empty) or into the file `path` (removed again when writing fails).
		void WriteVariants(const EventTable & table, size_t k, const ColorMap & map, const InputSequences & seq, const ColorTable & colors, const SuperbubbleTable & superbubbles,
			const VariantTable & variants, const std::string & path);

		// VCF 4.2 into the file `path`; needs a reference colour and the letters.  One record per site that has a traversal of the
		// reference and at least two alleles, ordered by (reference sequence, POS, site); ID sb<site>; REF the reference allele, read
		// from the reference traversal's own span, ALT the others in allele order, each spelled from its first traversal and turned to
		// the reference traversal's stored orientation; letters other than A C G T print as N.  Alleles of equal edges E >= k + 1 are
		// span[k : E] at POS = end[lo] + k + 1 (smaller equal edges exist only under an abundance cut); otherwise span[k - 1 : edges + k - min(k, Dmin)] at POS = end[lo] + k.  INFO: AC
		// (traversals per ALT), AN (the site's traversals), NS (colours with a traversal), INS (inside).  One sample per colour,
		// labelled as the PHYLIP matrix labels it; GT: the record's allele indices the colour walks, ascending, joined by '/', or '.'.
		// No further normalisation.
		void WriteVariantsVcf(const EventTable & table, size_t k, const ColorMap & map, const InputSequences & seq, const LoadedSequences & loaded, const ColorTable & colors,
			const SuperbubbleTable & superbubbles, const VariantTable & variants, const std::string & path);

		// Both files, or neither: the VCF first when vcfPath is given, then the TSV (to stdout when path is empty); when the TSV cannot
		// be written the VCF is removed again before the error is thrown.  loaded: may be 0 when vcfPath is empty.
		void WriteVariantFiles(const EventTable & table, size_t k, const ColorMap & map, const InputSequences & seq, const LoadedSequences * loaded, const ColorTable & colors,
			const SuperbubbleTable & superbubbles, const VariantTable & variants, const std::string & path, const std::string & vcfPath);

		// ---------------------------------------------------------------------------------------- the anchor blocks
		// Where the sequence a colour shares with a reference colour lies in both (include/twopaco_hip.h, the tpc_segments_anchors_*
		// group, states the definition in the same words).  count[r][c]: the events of row r in sequences of colour c.  An event e of
		// row r in colour c != ref is an ANCHOR when count[r][ref] == 1 and count[r][c] == 1; mate[e] is the one event of r in the
		// reference colour; the anchor is REVERSE when name[e] and name[mate[e]] differ in sign.  An anchor e CONTINUES e - 1 when both
		// lie in one sequence, e - 1 is an anchor with the same reverse flag, mate[e] == mate[e - 1] + 1 (forward) or - 1 (reverse),
		// and both mates lie in one reference sequence.  A BLOCK is a maximal run queryFirst .. queryLast of anchors each continuing
		// the one before; its reference events refFirst .. refLast ascend (reverse: mate[queryLast] .. mate[queryFirst]).  Blocks
		// ascend by queryFirst.  Per colour other than ref: blocks, anchors, edges (end[queryLast] - begin[queryFirst] summed) and
		// reverseEdges; refEdges is the sum of end - begin over the reference colour's events.  The arrays come from ComputeAnchors
		// below -- the serial statement -- or from the device (csrc/tpc_anchors.hip); the writers print either as the same bytes.
		struct AnchorTable
		{
			static const uint32_t NONE = 0xFFFFFFFFu;                      // mate[]: no mate
			uint64_t colors, segments, refEdges;
			uint32_t ref;
			std::vector<uint32_t> mate;                                    // [events]
			std::vector<uint32_t> queryFirst, queryLast, refFirst, refLast; // [blocks], events
			std::vector<uint64_t> blocks, anchors, edges, reverseEdges;     // [colors], 0 for ref
			AnchorTable() : colors(0), segments(0), refEdges(0), ref(0) {}
			size_t Rows() const { return queryFirst.size(); }
			uint64_t Anchors() const { uint64_t n = 0; for (uint64_t a : anchors) n += a; return n; }
		};

		// The definition stated with std:: containers: the row of every event by a hash map from |name|, count[][] as one std::map from
		// (row, colour) to the number of events and the last of them, the mates, then one pass over the events for the blocks.  The
		// table must be one whose walk did not fail; every sequence needs a colour below `colors`, and ref < colors
		// (std::runtime_error otherwise).  No device dependency.
		void ComputeAnchors(const EventTable & table, size_t k, const std::vector<uint32_t> & colorOfSequence, uint64_t colors, uint32_t ref, AnchorTable & out);

		// The TSV text: "#twopaco-anchors\t1\tby=<file|sequence>\tk=<k>\tcolors=<C>\tsegments=<S>\tref=<R>\tref_edges=<T>\tblocks=<B>", the
		// colour table's "#color" lines, "#sequence\t<s>\t<colour>\t<length>\t<name>" for every input sequence, "#shared\t<c>\t<blocks>\t
		// <anchors>\t<edges>\t<reverse_edges>" for every colour other than R, zeros included, then one line per block: colour, ref_seq,
		// ref_begin, ref_end, + or -, query_seq, query_begin, query_end, anchors.  Sequences are 0-based input indices, intervals
		// half-open, all coordinates on each sequence's forward strand.  To stdout (path empty) or into the file `path` (removed again
		// when writing fails).
		void WriteAnchors(const EventTable & table, size_t k, const ColorMap & map, const InputSequences & seq, const AnchorTable & anchors, const std::string & path);

		// PAF, one line per block in the table's order, into the file `path`: query name, length, begin, end, strand, reference name,
		// length, begin, end, matches (= the block length), the block length, 255, tp:A:P, cg:Z:<len>=, an:i:<anchors>.
		void WriteAnchorsPaf(const EventTable & table, size_t k, const ColorMap & map, const InputSequences & seq, const AnchorTable & anchors, const std::string & path);

		// Both files, or neither: the PAF first when pafPath is given, then the TSV (to stdout when path is empty); when the TSV cannot
		// be written the PAF file is removed again before the error is thrown.
		void WriteAnchorFiles(const EventTable & table, size_t k, const ColorMap & map, const InputSequences & seq, const AnchorTable & anchors, const std::string & path,
			const std::string & pafPath);

		// ---------------------------------------------------------------------------------------- the edge index and locate
		// Is a sequence that was no input in the graph, where, and in which colours (include/twopaco_hip.h, the tpc_segments_edges_* and
		// tpc_segments_locate_* groups, state the definition in the same words).  n = k + 1; T = N seq0 N seq1 N ... with every letter
		// other than A C G T an N; a window T[g, g + n) is valid when it holds no N; canon(w) is the smaller of w and its reverse
		// complement.  The SPAN of row r (the colour table's rows: first events in event order) is T[g0, g0 + end - begin) of its first
		// event, g0 = the sequence's start in T + begin.  The index holds canon(window) -> (g, row) for every span position with a valid
		// window, the SMALLEST g where positions share a key (the others are duplicates; span positions with an invalid window are
		// skipped).  ComputeLocate below is the serial statement: an unordered_map of canonical windows, no device.
		struct EdgeIndex
		{
			size_t k;
			std::string text;                                              // T
			std::vector<uint64_t> g0;                                      // [rows]
			std::unordered_map<std::string, std::pair<uint64_t, uint32_t> > entry;
			uint64_t duplicates, skipped;
			EdgeIndex() : k(0), duplicates(0), skipped(0) {}
		};

		// The table must be one whose walk did not fail and must have passed CheckEventTable against `loaded`.
		void BuildEdgeIndex(const EventTable & table, const LoadedSequences & loaded, size_t k, EdgeIndex & out);

		// Every window of every query record: invalid (it holds an N), absent (no key of the index) or a hit (g, row, rev), rev = 0 when
		// the window equals T's letter for letter (a palindrome counts as forward).  off = g - g0(row).  A hit CONTINUES the one before it
		// when both lie in one row with one rev and off steps by + 1 (forward) or - 1 (reverse); a RUN is a maximal chain, runs ascend by
		// query position.  Per record: windows (valid), found, forward (hits with rev = 0), runs, shared[c] (hits whose row has colour c).
		// The arrays come from ComputeLocate or from the device (csrc/tpc_locate.hip, devicegraph.h); the writers print either as the same bytes.
		struct LocateTable
		{
			uint64_t colors, segments, entries, duplicates;
			std::vector<uint64_t> windows, found, forward, runs;           // [queries]
			std::vector<uint64_t> shared;                                  // [queries][colors]
			std::vector<uint64_t> runQuery, runBegin;                      // [runs]: the record and the 0-based position of the first window on it
			std::vector<uint32_t> runLength, runRow, runRev, runOff;       // [runs]: windows, row, rev, off of the first window
			LocateTable() : colors(0), segments(0), entries(0), duplicates(0) {}
			size_t Queries() const { return windows.size(); }
			size_t Runs() const { return runQuery.size(); }
		};

		void ComputeLocate(const EdgeIndex & index, const ColorTable & colors, const LoadedSequences & queries, LocateTable & out);

		// The TSV text: "#twopaco-locate\t1\tby=<file|sequence>\tk=<k>\tcolors=<C>\tsegments=<S>\tentries=<E>\tduplicates=<D>\tqueries=<Q>", the
		// colour table's "#color" lines, one line per query record (name, length, windows, found, forward, runs, then C integers: the hits
		// in rows of each colour), "#total\t<windows>\t<found>\t<forward>\t<runs>".  To stdout (path empty) or into the file `path`.
		void WriteLocate(size_t k, const ColorMap & map, const InputSequences & queries, const LocateTable & locate, const std::string & path);

		// "#twopaco-locate-walks\t1\tk=<k>", then one line per run: query_index, q_begin, q_end (half-open, 0-based on the record, q_end =
		// q_begin + length + k), the segment as gfa1 names it, the strand, s_begin, s_end on the S line's body: where name[e0] < 0 the body
		// is the reverse complement of the span, so the offsets and the strand are flipped.
		void WriteLocateWalks(const EventTable & table, size_t k, const ColorTable & colors, const LocateTable & locate, const std::string & path);

		// Both files, or neither: the walks first when walksPath is given, then the TSV; when the TSV cannot be written the walks file is
		// removed again before the error is thrown.
		void WriteLocateFiles(const EventTable & table, size_t k, const ColorMap & map, const ColorTable & colors, const InputSequences & queries, const LocateTable & locate,
			const std::string & path, const std::string & walksPath);

		// Header lines and events into the file outPath (created or truncated; removed again when anything fails); compact when
		// the table carries linkFirst.
		void WriteGraphFile(const EventTable & table, const InputSequences & seq, const LoadedSequences & loaded, size_t k, const std::string & format,
			size_t threads, const std::string & outPath);
	}
}

#endif
