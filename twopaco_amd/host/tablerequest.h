// tablerequest.h -- "this run wants these tables of the compacted graph, of these colours, into these files", said once for both
// programs: the request (TableRequest), one static row per table (TABLE_ROWS: its flag, the noun of its messages, its options, its
// default file name, what it reads), the rules of what a request needs derived from those rows, the command-line options of the
// tables and their complaints (ParseTableOption, CheckTableOptions; what differs between `graphdump` and `twopaco` is TableCliRules,
// data), and the serial pipeline and the writer (Tables, ComputeTables, WriteTables).  The device pipeline over the same request is
// devicegraph.h's BuildTables.
#ifndef _TABLE_REQUEST_H_
#define _TABLE_REQUEST_H_

#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "graphformat.h"

namespace TwoPaCo
{
	namespace GraphFormat
	{
		// in the order the tables are written
		enum TableId { COLORS, LINKS, BUBBLES, DISTANCES, COMPONENTS, SUPERBUBBLES, ANCHORS, LOCATE, CLASSES, TRACKS, VARIANTS, TABLES };

		enum Reads { NOTHING, BUILD, ROWS };  // of a device stage: not read, built and read where it lies, its rows fetched for the files

		struct TableRow
		{
			const char * name;        // --<name> [file|sequence], --<name>-out, de_bruijn.<name>.tsv
			const char * noun;        // "The <noun> table ..."
			bool colours;             // takes file|sequence (the link table has no colours)
			const char * second;      // --<name>-<second>: the second file, or 0
			const char * secondNoun;  // what the second file holds, and whether that is a plural
			bool secondPlural;
			const char * extra;       // the option beside them that is nothing without the table, or 0
			Reads colorStage, linkStage;
			bool events, letters;     // prints names, lengths or positions of the event table; reads the input's letters
		};

		const TableRow TABLE_ROWS[TABLES] =
		{
			{"colors", "colour", true, 0, 0, false, 0, ROWS, NOTHING, true, false},
			{"links", "link", false, 0, 0, false, 0, NOTHING, ROWS, true, false},
			{"bubbles", "bubble", true, 0, 0, false, 0, ROWS, BUILD, true, false},
			{"distances", "distance", true, "phylip", "The PHYLIP matrix", false, 0, BUILD, NOTHING, false, false},
			{"components", "component", true, "members", "The component members", true, 0, ROWS, BUILD, true, false},
			{"superbubbles", "superbubble", true, "members", "The superbubble members", true, "--superbubbles-max", ROWS, BUILD, true, false},
			{"anchors", "anchor", true, "paf", "The anchor PAF", false, "--anchors-ref", NOTHING, NOTHING, true, false},
			{"locate", "locate", true, "walks", "The locate walks", true, "--locate-in", ROWS, NOTHING, true, true},
			{"classes", "class", true, "members", "The class members", true, 0, ROWS, NOTHING, true, false},
			{"tracks", "track", true, "bedgraph", "The track bedGraph", false, "--tracks-of", ROWS, NOTHING, true, false},
			{"variants", "variant", true, "vcf", "The variant VCF", false, "--variants-ref", ROWS, BUILD, true, true},
		};

		struct TableRequest
		{
			struct File
			{
				bool on;
				std::string out, second;  // out empty: the standard output (graphdump); second empty: no second file
				File() : on(false) {}
			};

			File table[TABLES];
			bool bySequence;                    // the colours of all tables: the input's sequences, or its files
			uint32_t superbubblesMax, anchorsRef;
			uint32_t tracksOf;                  // the one colour of the track table, TrackTable::ALL: every colour
			uint32_t variantsRef;               // the reference colour of the variant table, VariantTable::NONE: none
			std::vector<std::string> locateIn;  // the FASTA files of the queries
			TableRequest() : bySequence(false), superbubblesMax(62), anchorsRef(0), tracksOf(TrackTable::ALL), variantsRef(VariantTable::NONE) {}

			bool On(TableId t) const { return table[t].on; }
			bool Any() const
			{
				for (int t = 0; t < TABLES; t++) if (table[t].on) return true;
				return false;
			}
		};

	}

	// (hidden: every program compiles its own copy, libtwopaco_host.so exports none of it)
	namespace GraphFormat __attribute__((visibility("hidden")))
	{
		// what a request needs, from the rows
		inline bool ReadsAtLeast(const TableRequest & r, Reads TableRow::*stage, Reads least)
		{
			for (int t = 0; t < TABLES; t++) if (r.table[t].on && TABLE_ROWS[t].*stage >= least) return true;
			return false;
		}

		inline bool NeedsColorBuild(const TableRequest & r) { return ReadsAtLeast(r, &TableRow::colorStage, BUILD); }
		inline bool NeedsColorRows(const TableRequest & r) { return ReadsAtLeast(r, &TableRow::colorStage, ROWS); }
		inline bool NeedsLinkBuild(const TableRequest & r) { return ReadsAtLeast(r, &TableRow::linkStage, BUILD); }
		inline bool NeedsLinkRows(const TableRequest & r) { return ReadsAtLeast(r, &TableRow::linkStage, ROWS); }
		inline bool NeedsColorMap(const TableRequest & r) { return NeedsColorBuild(r) || r.On(ANCHORS); }
		// the superbubble table is built for its own files and for the variant table, which walks the genomes through its rows
		inline bool NeedsSuperbubbleBuild(const TableRequest & r) { return r.On(SUPERBUBBLES) || r.On(VARIANTS); }
		inline bool NeedsEventTable(const TableRequest & r)
		{
			for (int t = 0; t < TABLES; t++) if (r.table[t].on && TABLE_ROWS[t].events) return true;
			return false;
		}

		inline bool NeedsLetters(const TableRequest & r)
		{
			for (int t = 0; t < TABLES; t++) if (r.table[t].on && TABLE_ROWS[t].letters) return true;
			return false;
		}

		inline std::string TableNoun(int t) { return std::string("The ") + TABLE_ROWS[t].noun + " table"; }

		// The complaint about two tables of different colours, for the command lines and for CreateEnumerator's C callers; how: what
		// was given, or what is asked for
		inline std::string SharedColoursComplaint(int later, const std::string & earlierNoun, const std::string & how)
		{
			return TableNoun(later) + " and the " + earlierNoun + " share one set of colours: " + how;
		}

		// The request as strings give it (CreateEnumerator's C callers): table t into `file` (and `second`), its colours `by` file |
		// sequence, the same for every table that has colours.  The colour table is wanted when `by` is given, every other table when
		// `file` is.
		inline void SetTable(TableRequest & r, TableId t, const char * by, const char * file, const char * second)
		{
			const std::string mode = by ? by : "";
			r.table[t].out = file ? file : "";
			r.table[t].second = second ? second : "";
			r.table[t].on = t == COLORS ? !mode.empty() : !r.table[t].out.empty();
			if (!r.table[t].on || !TABLE_ROWS[t].colours) return;
			if (mode != "file" && mode != "sequence") throw std::runtime_error((t == COLORS ? std::string("The colours") : TableNoun(t) + "'s colours") + " must be one of file, sequence");
			for (int e = 0; e < t; e++)
			{
				if (r.table[e].on && TABLE_ROWS[e].colours && r.bySequence != (mode == "sequence"))
				{
					throw std::runtime_error(SharedColoursComplaint(t, std::string(TABLE_ROWS[e].noun) + " table", "both by file or both by sequence"));
				}
			}

			r.bySequence = mode == "sequence";
		}

		// ------------------------------------------------------------------------------------------------ the command line
		struct ArgError : public std::runtime_error
		{
			std::string arg;
			ArgError(const std::string & msg, const std::string & argId) : std::runtime_error(msg), arg(argId) {}
		};

		// the tables' options as one command line gave them
		struct TableOptions
		{
			TableRequest request;
			std::string by[TABLES];  // file | sequence as given; empty: not given
			bool outSet[TABLES], secondSet[TABLES], extraSet[TABLES];
			TableOptions() : outSet(), secondSet(), extraSet() {}
		};

		// What differs between the two programs' command lines.
		struct TableCliRules
		{
			const char * constraintTag;   // in front of "(--flag)" where a value does not meet its constraint
			int order[TABLES];            // the tables in the order their complaints are looked for
			bool queryOrphanFirst;        // --locate-in without --locate is complained of before --locate-out (else after --locate-walks)
			// graphdump: a table instead of -f, some tables one at a time, all formatted by the host
			bool haveFormat, compact, textSet;
			unsigned apart[TABLES];       // bit e: table t is not written beside the earlier table e
			bool apartFromCompact[TABLES];
			// twopaco: one GPU, a file name for every table, the colours known when they are the files
			int gpus;
			bool defaultFiles;
			size_t inputFiles;
		};

		inline long ParseBounded(const std::string & v, long long low, long long high, const char * constraint, const std::string & tag)
		{
			char * end = 0;
			const long long n = std::strtoll(v.c_str(), &end, 10);
			if (v.empty() || *end || n < low || n > high) throw ArgError("Value '" + v + "' does not meet constraint: " + constraint, tag);
			return long(n);
		}

		// One argument of the command line that belongs to a table, with its value from value("(--flag)"); false: not a table's.
		template<class Value> bool ParseTableOption(const std::string & a, Value value, const char * constraintTag, TableOptions & o)
		{
			if (a.compare(0, 2, "--") != 0) return false;
			const std::string tag = "(" + a + ")";
			if (a == "--superbubbles-max") o.request.superbubblesMax = uint32_t(ParseBounded(value(tag), 2, 62, "an integer 2 .. 62", constraintTag + tag));
			else if (a == "--anchors-ref") o.request.anchorsRef = uint32_t(ParseBounded(value(tag), 0, 0x7FFFFFFFll, "a colour index", constraintTag + tag));
			else if (a == "--locate-in") o.request.locateIn.push_back(value(tag));
			else if (a == "--tracks-of") o.request.tracksOf = uint32_t(ParseBounded(value(tag), 0, 0x7FFFFFFFll, "a colour index", constraintTag + tag));
			else if (a == "--variants-ref") o.request.variantsRef = uint32_t(ParseBounded(value(tag), 0, 0x7FFFFFFFll, "a colour index", constraintTag + tag));
			for (int t = 0; t < TABLES; t++)
			{
				const TableRow & row = TABLE_ROWS[t];
				const std::string flag = std::string("--") + row.name;
				if (row.extra && a == row.extra) o.extraSet[t] = true;
				else if (a == flag && row.colours)
				{
					o.by[t] = value(tag);
					if (o.by[t] != "file" && o.by[t] != "sequence") throw ArgError("Value '" + o.by[t] + "' does not meet constraint: file|sequence", constraintTag + tag);
					o.request.table[t].on = true;
				}
				else if (a == flag) o.request.table[t].on = true;
				else if (a == flag + "-out") { o.request.table[t].out = value(tag); o.outSet[t] = true; }
				else if (row.second && a == flag + "-" + row.second) { o.request.table[t].second = value(tag); o.secondSet[t] = true; }
				else continue;
				return true;
			}

			return false;
		}

		// Every complaint about the tables' options together, the first one thrown; then the request's colours.
		inline void CheckTableOptions(TableOptions & o, const TableCliRules & rules)
		{
			TableRequest & r = o.request;
			for (int at = 0; at < TABLES; at++)
			{
				const int t = rules.order[at];
				const TableRow & row = TABLE_ROWS[t];
				TableRequest::File & file = r.table[t];
				const std::string flag = std::string("--") + row.name, tag = "(" + flag + ")";
				if (!file.on)
				{
					// (--superbubbles-max is the variant table's as well)
					const bool orphan[3] = {o.outSet[t], o.secondSet[t], o.extraSet[t] && !(t == SUPERBUBBLES && r.table[VARIANTS].on)};
					const std::string option[3] = {flag + "-out", row.second ? flag + "-" + row.second : "", row.extra ? row.extra : ""};
					const int first = rules.queryOrphanFirst && t == LOCATE ? 2 : 0;
					for (int i = 0; i < 3; i++)
					{
						const int which = (first + i) % 3;
						if (orphan[which]) throw ArgError("This argument needs " + flag + (row.colours ? " <file|sequence>" : ""), "(" + option[which] + ")");
					}

					continue;
				}

				if (rules.haveFormat) throw ArgError("Mutually exclusive argument already set!", tag);
				if (rules.gpus > 1) throw ArgError(TableNoun(t) + " is written by one GPU only (every rank holds its own piece of the junction stream): not with --gpus above 1", tag);
				for (int e = 0; e < t; e++)
				{
					if (r.table[e].on && TABLE_ROWS[e].colours && row.colours && !(rules.apart[t] >> e & 1) && o.by[e] != o.by[t])
					{
						throw ArgError(SharedColoursComplaint(t, std::string(TABLE_ROWS[e].noun) + " table", "--" + std::string(TABLE_ROWS[e].name) + " " + o.by[e] + " does not go with " + flag + " " + o.by[t]), tag);
					}
				}

				for (int e = 0; e < t; e++)
				{
					if (r.table[e].on && (rules.apart[t] >> e & 1)) throw ArgError(TableNoun(t) + " and the " + TABLE_ROWS[e].noun + " table are written one at a time: not with --" + TABLE_ROWS[e].name, tag);
				}

				if (rules.compact && rules.apartFromCompact[t]) throw ArgError(TableNoun(t) + " and the compact text are written one at a time: not with --compact", tag);
				if (rules.textSet) throw ArgError(TableNoun(t) + " is formatted by the host: not with " + flag, "(--text)");
				if (t == LOCATE && r.locateIn.empty()) throw ArgError("The locate table needs a query: --locate-in <fasta file>", tag);
				if (rules.defaultFiles)
				{
					if (!o.outSet[t]) file.out = std::string("de_bruijn.") + row.name + ".tsv";
					// (an empty name for the colour table is CreateEnumerator's to refuse)
					if (file.out.empty() && t != COLORS) throw ArgError(TableNoun(t) + " needs a file name", "(" + flag + "-out)");
				}

				if (o.secondSet[t] && file.second.empty()) throw ArgError(std::string(row.secondNoun) + (row.secondPlural ? " need" : " needs") + " a file name", "(" + flag + "-" + row.second + ")");
				if (t == ANCHORS && rules.inputFiles && o.by[t] == "file" && r.anchorsRef >= rules.inputFiles)
				{
					throw ArgError("Value '" + std::to_string(r.anchorsRef) + "' does not meet constraint: a colour index below " + std::to_string(rules.inputFiles), "(--anchors-ref)");
				}

				if (t == TRACKS && rules.inputFiles && o.by[t] == "file" && r.tracksOf != TrackTable::ALL && r.tracksOf >= rules.inputFiles)
				{
					throw ArgError("Value '" + std::to_string(r.tracksOf) + "' does not meet constraint: a colour index below " + std::to_string(rules.inputFiles), "(--tracks-of)");
				}

				if (t == VARIANTS && o.secondSet[t] && !o.extraSet[t]) throw ArgError("The variant VCF needs a reference colour: --variants-ref <integer>", "(" + flag + "-" + row.second + ")");
				if (t == VARIANTS && rules.inputFiles && o.by[t] == "file" && r.variantsRef != VariantTable::NONE && r.variantsRef >= rules.inputFiles)
				{
					throw ArgError("Value '" + std::to_string(r.variantsRef) + "' does not meet constraint: a colour index below " + std::to_string(rules.inputFiles), "(--variants-ref)");
				}
			}

			for (int t = TABLES; t-- > 0;) if (r.table[t].on && TABLE_ROWS[t].colours) r.bySequence = o.by[t] == "sequence";
		}

		// ------------------------------------------------------------------------------------------------ the tables of one run
		struct Tables
		{
			ColorMap map;
			ColorTable colors;
			LinkTable links;
			BubbleTable bubbles;
			DistanceTable distances;
			ComponentTable components;
			SuperbubbleTable superbubbles;
			AnchorTable anchors;
			LocateTable locate;
			ClassTable classes;
			TrackTable tracks;
			VariantTable variants;
			const LoadedSequences * letters; // of the input, for the variant VCF: the caller's, 0 when they were not loaded
			InputSequences queries;         // of request.locateIn
			LoadedSequences queryLetters;
			uint64_t segments, linkRows;    // the rows of the colour table and of the link table, fetched or not
			Tables() : letters(0), segments(0), linkRows(0) {}
		};

		inline void LoadQueries(const TableRequest & request, size_t threads, Tables & t)
		{
			if (request.On(LOCATE)) LoadSequences(request.locateIn, false, threads, t.queries, t.queryLetters);
		}

		// The serial pipeline: the Compute* statements the request needs over an event table, in the order of their dependencies.  t.map
		// is the caller's (MakeColorMap), and so are the queries (LoadQueries); loaded: the letters, read by --locate alone.
		inline void ComputeTables(const EventTable & table, const LoadedSequences & loaded, size_t k, const TableRequest & request, Tables & t)
		{
			for (uint64_t w = 0; w < (table.events + 31) / 32; w++) t.segments += uint64_t(__builtin_popcount(table.first[w]));
			if (NeedsColorBuild(request)) ComputeColors(table, k, t.map.colorOfSequence, t.map.label.size(), t.colors);
			if (NeedsLinkBuild(request)) ComputeLinks(table, t.links);
			t.linkRows = t.links.Rows();
			if (request.On(BUBBLES)) ComputeBubbles(table, t.links, t.bubbles);
			if (request.On(DISTANCES)) ComputeDistances(table, t.colors, t.distances);
			if (request.On(COMPONENTS)) ComputeComponents(table, k, t.links, t.colors, t.components);
			if (NeedsSuperbubbleBuild(request)) ComputeSuperbubbles(table, k, t.links, t.colors, request.superbubblesMax, t.superbubbles);
			if (request.On(ANCHORS)) ComputeAnchors(table, k, t.map.colorOfSequence, t.map.label.size(), request.anchorsRef, t.anchors);
			if (request.On(LOCATE))
			{
				CheckEventTable(table, loaded, k, 1);
				EdgeIndex index;
				BuildEdgeIndex(table, loaded, k, index);
				ComputeLocate(index, t.colors, t.queryLetters, t.locate);
			}

			if (request.On(CLASSES)) ComputeClasses(table, k, t.colors, t.classes);
			if (request.On(TRACKS)) ComputeTracks(table, k, t.map.colorOfSequence, t.map.label.size(), t.colors, request.tracksOf, t.tracks);
			if (request.On(VARIANTS)) ComputeVariants(table, k, t.map.colorOfSequence, t.map.label.size(), t.colors, t.superbubbles, request.variantsRef, t.variants);
		}

		// One table's files, if it is wanted
		inline void WriteTable(int id, const EventTable & table, size_t k, const TableRequest & request, const InputSequences & seq, const Tables & t)
		{
			const TableRequest::File & f = request.table[id];
			if (!f.on) return;
			switch (id)
			{
			case COLORS: WriteColors(table, k, t.map, t.colors, f.out); break;
			case LINKS: WriteLinks(table, k, t.segments, t.links, f.out); break;
			case BUBBLES: WriteBubbles(table, k, t.map, t.colors, t.linkRows, t.bubbles, f.out); break;
			case DISTANCES: WriteDistanceFiles(k, t.map, t.segments, t.distances, f.out, f.second); break;
			case COMPONENTS: WriteComponentFiles(table, k, t.map, t.colors, t.linkRows, t.components, f.out, f.second); break;
			case SUPERBUBBLES: WriteSuperbubbleFiles(table, k, t.map, t.colors, t.linkRows, t.superbubbles, f.out, f.second); break;
			case ANCHORS: WriteAnchorFiles(table, k, t.map, seq, t.anchors, f.out, f.second); break;
			case LOCATE: WriteLocateFiles(table, k, t.map, t.colors, t.queries, t.locate, f.out, f.second); break;
			case CLASSES: WriteClassFiles(table, k, t.map, t.colors, t.classes, f.out, f.second); break;
			case TRACKS: WriteTrackFiles(table, k, t.map, seq, t.colors, t.tracks, f.out, f.second); break;
			case VARIANTS: WriteVariantFiles(table, k, t.map, seq, t.letters, t.colors, t.superbubbles, t.variants, f.out, f.second); break;
			}
		}

		// The wanted tables from `first` on, in the established order; written(id) after each one that was
		template<class Written> void WriteTables(int first, const EventTable & table, size_t k, const TableRequest & request, const InputSequences & seq, const Tables & t, Written written)
		{
			for (int id = first; id < TABLES; id++)
			{
				WriteTable(id, table, k, request, seq, t);
				if (request.table[id].on) written(id);
			}
		}
	}
}

#endif
