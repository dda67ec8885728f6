// constructor.cpp -- the `twopaco` command line, flag-compatible with the reference CLI
// (reference src/graphconstructor/constructor.cpp:53-218): -k/--kvalue (odd, default 25),
// -f/--filtersize xor --filtermemory (GB; bits = log2(GB*8e9) truncated, :158; `-f auto`, not in the reference: the size from a
// sketch of the input's distinct edges, filterplan.h), -q/--hashfnumber
// (5), -r/--rounds (1), -t/--threads (1), -a/--abundance (UINT64_MAX), --tmpdir ("."),
// -o/--outfile ("de_bruijn.bin"), --test, and the FASTA file names.  Extra flags that do not
// exist in the reference: --seed S (pin the hash tables, see seed.h), --device N,
// --test-first (test-then-set insert), --gpus N (Bloom filter sharded by bit address over N GPUs of the node,
// RCCL between them; --no-rccl: device-to-device copies; --emulate-ranks: N ranks on one device, for testing),
// --save-filter F / --load-filter F (checkpoint of the Bloom filter after each round's first-pass insert, the reference's
// commented-out ReloadBloomFilter, vertexenumerator.h:29,113-121; a run that loads skips the insert), and with --test,
// --seed makes the trials reproducible (the reference's are not, test.cpp:169);
// --graph gfa1|gfa2|fasta [--graph-out F] [--graph-prefix] [--graph-threads N] [--graph-text host|device]: the compacted graph as text from this process,
// byte for byte what `graphdump -f <format> [--prefix]` prints for the junction stream of the same command (graphformat.h; the
// stream stays on the device and the junction file is written only when -o is given as well; one GPU; --graph-text device renders
// the text on the device too, csrc/tpc_segtext.hip, instead of fetching the event table and formatting it here);
// --colors file|sequence [--colors-out F]: the segment colour table of the same graph -- which input files, or sequences, hold
// each segment, how often, on which strand -- as TSV, byte for byte what `graphdump --colors` writes for the junction stream of
// the same command (csrc/tpc_colors.hip groups the events on the device; combines with --graph and -o, the segment table is
// built once; one GPU);
// --links [--links-out F]: the link table of the same graph -- every distinct link once with its occurrences -- as TSV, byte for
// byte what `graphdump --links` writes (csrc/tpc_links.hip finds the links on the device; combines with --graph, --colors and -o);
// --graph-compact: with --graph gfa1 the text `graphdump -f gfa1 --compact` prints, every link once;
// --bubbles file|sequence [--bubbles-out F]: the simple bubbles of the same graph -- where two segments leave one side of a segment,
// touch nothing else and meet again -- with the colours of the two arms, as TSV, byte for byte what `graphdump --bubbles` writes
// (csrc/tpc_bubbles.hip finds them on the device over the link table; combines with --graph, --graph-compact, --colors, --links
// and -o from one segment, colour and link build; --colors must name the same colours);
// --distances file|sequence [--distances-out F] [--distances-phylip F]: how much every colour shares with every other one -- the
// segments and the edges ((k+1)-mers) two colours both hold -- as TSV of integers, byte for byte what `graphdump --distances` writes,
// and asked for, the Jaccard distances over edges as a PHYLIP square matrix (csrc/tpc_distances.hip sums the matrices on the device
// over the colour build; combines with everything above from one segment build and one colour build; --colors and --bubbles must
// name the same colours; its file is written last);
// --components file|sequence [--components-out F] [--components-members F]: the connected components of the same graph -- which
// segments hang together -- as TSV of integers, byte for byte what `graphdump --components` writes, and asked for, the component of
// every segment (csrc/tpc_components.hip finds them on the device over the link build and the colour build; combines with everything
// above from one segment, colour and link build; --colors, --bubbles and --distances must name the same colours; its files are
// written after the distance files);
// --superbubbles file|sequence [--superbubbles-out F] [--superbubbles-members F] [--superbubbles-max N]: the superbubbles of the same
// graph, bounded to N sides inside (2 .. 62, default 62) -- where the genomes differ beyond two alleles -- as TSV of integers, byte
// for byte what `graphdump --superbubbles` writes, and asked for, the inside sides of every row (csrc/tpc_superbubbles.hip finds them
// on the device over the link build and the colour build; combines with everything above from one segment, colour and link build;
// the other tables must name the same colours; its files are written after the component files);
// --anchors file|sequence [--anchors-ref N] [--anchors-out F] [--anchors-paf F]: the anchor blocks of every other colour against the
// reference colour N (default 0) -- unique collinear matches, forward or reverse-complement -- as TSV, byte for byte what `graphdump
// --anchors` writes, and asked for, as PAF (csrc/tpc_anchors.hip finds them on the device over the event table of the same segment
// build; combines with everything above; the other tables must name the same colours; its files are written after the superbubble files);
// --locate file|sequence --locate-in Q.fa [--locate-in ...] [--locate-out F] [--locate-walks F]: the records of the query files looked
// up in the graph window by window -- found, where, on which strand, in which colours -- as TSV, byte for byte what `graphdump
// --locate` writes, and asked for, the runs as a walks file (csrc/tpc_locate.hip builds the edge index and looks the queries up on
// the device; combines with everything above; the other tables must name the same colours; its files are written after the anchor files);
// --classes file|sequence [--classes-out F] [--classes-members F]: the colour classes of the same graph -- the distinct sets of colours
// and the segments that have each -- as TSV of integers, byte for byte what `graphdump --classes` writes, and asked for, the class of
// every segment (csrc/tpc_classes.hip groups the colour rows on the device; combines with everything above from one segment and colour
// build; the other tables must name the same colours; its files are written after the locate files);
// --tracks file|sequence [--tracks-of N] [--tracks-out F] [--tracks-bedgraph F]: the presence tracks of the input sequences -- for
// every stretch of every sequence the colours that share it -- as TSV of integers, byte for byte what `graphdump --tracks` writes, and
// asked for, a bedGraph of the number of colours (csrc/tpc_tracks.hip projects the colour rows onto the events on the device; combines
// with everything above from one segment and colour build; the same colours; its files are written after the class files);
// --variants file|sequence [--variants-ref N] [--variants-out F] [--variants-vcf F]: the alleles every genome walks through every
// superbubble as TSV of integers, byte for byte what `graphdump --variants` writes, and with a reference colour, as VCF 4.2
// (csrc/tpc_variants.hip walks the events on the device; combines with everything above from one segment, colour, link and
// superbubble build; the same colours; its files are written last).  Errors go to stderr as "\nError: <what>\n", exit code 1
// (reference constructor.cpp:179-188).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <unistd.h>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "selftest.h"
#include "vertexenumerator.h"

namespace
{
	using TwoPaCo::GraphFormat::ArgError;

	bool Match(const std::string & a, const char * shortName, const char * longName)
	{
		return (shortName && a == std::string("-") + shortName) || (longName && a == std::string("--") + longName);
	}

	template<class T> T Parse(const std::string & text, const std::string & argId)
	{
		try
		{
			size_t used = 0;
			if (text.empty() || text[0] == '-') throw std::invalid_argument(text);
			unsigned long long v = std::stoull(text, &used, 10);
			if (used != text.size()) throw std::invalid_argument(text);
			return static_cast<T>(v);
		}
		catch (std::exception &)
		{
			throw ArgError("Couldn't read argument value from string '" + text + "'", argId);
		}
	}

	void Usage()
	{
		std::cout << "USAGE: twopaco {-f <integer|auto>|--filtermemory <float>} [-k <oddc>] [-q <integer>] [-r <integer>]" << std::endl
			<< "               [-t <integer>] [-a <integer>] [--tmpdir <directory name>] [-o <file name>] [--test]" << std::endl
			<< "               [--seed <integer>] [--device <integer>] [--test-first] [--gpus <power of two>] [--no-rccl]" << std::endl
			<< "               [--save-filter <file>] [--load-filter <file>]" << std::endl
			<< "               [--graph <gfa1|gfa2|fasta>] [--graph-out <file name>] [--graph-prefix] [--graph-threads <integer>]" << std::endl
			<< "               [--graph-text <host|device>]" << std::endl
			<< "               [--colors <file|sequence>] [--colors-out <file name>]" << std::endl
			<< "               [--links] [--links-out <file name>] [--graph-compact]" << std::endl
			<< "               [--bubbles <file|sequence>] [--bubbles-out <file name>]" << std::endl
			<< "               [--distances <file|sequence>] [--distances-out <file name>] [--distances-phylip <file name>]" << std::endl
			<< "               [--components <file|sequence>] [--components-out <file name>] [--components-members <file name>]" << std::endl
			<< "               [--superbubbles <file|sequence>] [--superbubbles-out <file name>] [--superbubbles-members <file name>] [--superbubbles-max <integer>]" << std::endl
			<< "               [--anchors <file|sequence>] [--anchors-ref <integer>] [--anchors-out <file name>] [--anchors-paf <file name>]" << std::endl
			<< "               [--locate <file|sequence> --locate-in <file name> ... [--locate-out <file name>] [--locate-walks <file name>]]" << std::endl
			<< "               [--classes <file|sequence>] [--classes-out <file name>] [--classes-members <file name>]" << std::endl
			<< "               [--tracks <file|sequence>] [--tracks-of <integer>] [--tracks-out <file name>] [--tracks-bedgraph <file name>]" << std::endl
			<< "               [--variants <file|sequence>] [--variants-ref <integer>] [--variants-out <file name>] [--variants-vcf <file name>]" << std::endl
			<< "               <fasta files with genomes> ..." << std::endl
			<< "       -f auto: the filter size (and, without -r, the rounds) from a count of the input's distinct edges taken on the GPU" << std::endl
			<< "               (one GPU; not with --load-filter or --test)" << std::endl
			<< "       -q: 1..64 hash functions (the reference takes any number; more than 16 run on slower closed-form kernels)" << std::endl
			<< "       --graph: also write the compacted graph as graphdump -f <format> prints it, to --graph-out (default" << std::endl
			<< "               de_bruijn.<format>); the junction file is then written only when -o is given.  --graph-prefix:" << std::endl
			<< "               graphdump's --prefix.  --graph-threads: formatting threads (1..16, default 16).  One GPU only." << std::endl
			<< "               --graph-text: host (default) formats the text with the threads above; device renders the same bytes" << std::endl
			<< "               on the GPU, the host only writes them (--graph-threads is then unused)" << std::endl
			<< "       --colors: also write the segment colour table of the graph as TSV to --colors-out (default de_bruijn.colors.tsv):" << std::endl
			<< "               per segment its length, occurrences, forward occurrences, number of colours and presence bits, a colour" << std::endl
			<< "               being the c-th input file or the c-th sequence; then the histogram of segments by number of colours." << std::endl
			<< "               Combines with --graph and -o.  One GPU only." << std::endl
			<< "       --links: also write the link table of the graph as TSV to --links-out (default de_bruijn.links.tsv): every distinct" << std::endl
			<< "               link between two segments once, as spelled where it is first met, its occurrences and how many of them" << std::endl
			<< "               are spelled that way (a b and -b -a are one link).  Combines with --graph, --colors and -o.  One GPU only." << std::endl
			<< "       --graph-compact: with --graph gfa1, the compact text: no per-sequence S lines, no C lines, every link once (what" << std::endl
			<< "               graphdump -f gfa1 --compact prints).  Not with --graph-text device.  One GPU only." << std::endl
			<< "       --bubbles: also write the simple bubbles of the graph as TSV to --bubbles-out (default de_bruijn.bubbles.tsv): where" << std::endl
			<< "               two segments leave one side of a segment, touch nothing else and meet again at one side of another -- a" << std::endl
			<< "               substitution or a short insertion or deletion between genomes.  Per bubble its source, arms and sink, the arms'" << std::endl
			<< "               lengths, occurrences and colours (by file or by sequence, as --colors) and the colours that hold both arms." << std::endl
			<< "               Simple bubbles only: three alleles at one place, nested bubbles and superbubbles are not reported." << std::endl
			<< "               Combines with --graph, --graph-compact, --colors (the same colours), --links and -o.  One GPU only." << std::endl
			<< "       --distances: also write how much every colour (file or sequence, as --colors) shares with every other one as TSV to" << std::endl
			<< "               --distances-out (default de_bruijn.distances.tsv): per colour its own segments and edges ((k+1)-mers), then for" << std::endl
			<< "               every pair i < j the segments and the edges both hold; integers only, Jaccard = e_ij / (e_ii + e_jj - e_ij)." << std::endl
			<< "               --distances-phylip: also the Jaccard distances over edges as a relaxed PHYLIP square matrix." << std::endl
			<< "               Combines with --graph, --graph-compact, --colors and --bubbles (the same colours), --links and -o.  One GPU only." << std::endl
			<< "       --components: also write the connected components of the graph as TSV to --components-out (default" << std::endl
			<< "               de_bruijn.components.tsv): which segments hang together, a segment that no link touches being a component of one." << std::endl
			<< "               Per component the name of its first segment, its segments, links, bases, edges, occurrences and colours (by file" << std::endl
			<< "               or by sequence, as --colors).  --components-members: also the component of every segment, one line per segment." << std::endl
			<< "               Combines with --graph, --graph-compact, --colors, --bubbles and --distances (the same colours), --links and -o." << std::endl
			<< "               One GPU only." << std::endl
			<< "       --superbubbles: also write the superbubbles of the graph as TSV to --superbubbles-out (default" << std::endl
			<< "               de_bruijn.superbubbles.tsv): where the paths that leave one side of a segment meet again at one side of another" << std::endl
			<< "               and touch nothing else -- three alleles, substitutions closer than k, a substitution beside an indel, nested ones." << std::endl
			<< "               Per row entrance and exit, the sides inside, arcs, paths, the smallest and largest path weight in edges and the" << std::endl
			<< "               colours over the inside (by file or by sequence, as --colors).  --superbubbles-members: also the inside sides of" << std::endl
			<< "               every row.  --superbubbles-max: the largest inside reported, 2 .. 62 (default 62).  Combines with --graph," << std::endl
			<< "               --graph-compact, --colors, --bubbles, --distances and --components (the same colours), --links and -o.  One GPU only." << std::endl
			<< "       --anchors: also write the anchor blocks against the reference colour --anchors-ref (default 0) as TSV to --anchors-out (default" << std::endl
			<< "               de_bruijn.anchors.tsv): a segment that occurs exactly once in the reference and exactly once in another colour (by" << std::endl
			<< "               file or by sequence, as --colors) is an anchor, anchors that follow each other in both are chained into maximal" << std::endl
			<< "               collinear blocks, exact matches or exact reverse-complement matches between two intervals.  --anchors-paf: also the" << std::endl
			<< "               blocks as PAF.  Combines with --graph, --graph-compact, --colors, --bubbles, --distances, --components and" << std::endl
			<< "               --superbubbles (the same colours), --links and -o.  One GPU only." << std::endl
			<< "       --locate: also look every (k+1)-mer of the records of the --locate-in FASTA files up in the graph and write per record its valid" << std::endl
			<< "               windows, those found, those found forward, the runs they form and per colour (by file or by sequence, as --colors) the" << std::endl
			<< "               hits in segments of that colour as TSV to --locate-out (default de_bruijn.locate.tsv).  --locate-walks: also the runs," << std::endl
			<< "               one line each: the query's interval and the segment's.  Combines with all tables above (the same colours).  One GPU only." << std::endl
			<< "       --classes: also write the colour classes of the graph as TSV to --classes-out (default de_bruijn.classes.tsv): the distinct sets" << std::endl
			<< "               of colours (by file or by sequence, as --colors) that segments have, numbered in the order gfa1 first prints a segment of" << std::endl
			<< "               each.  Per class the name of its first segment, its segments, bases, edges, occurrences, number of colours and presence" << std::endl
			<< "               bits; in front the classes, segments and edges by number of colours.  --classes-members: also the class of every segment," << std::endl
			<< "               one line per segment.  Combines with all tables above (the same colours).  One GPU only." << std::endl
			<< "       --tracks: also write the presence tracks of the input sequences as TSV to --tracks-out (default de_bruijn.tracks.tsv): for every" << std::endl
			<< "               stretch of every sequence the colours (by file or by sequence, as --colors) that share it, neighbouring segment occurrences" << std::endl
			<< "               of equal presence merged into one interval: sequence, begin, end, occurrences, number of colours and presence bits; in" << std::endl
			<< "               front per colour its intervals, edges, core and private edges, and the intervals and edges by number of colours." << std::endl
			<< "               --tracks-of: the sequences of this one colour only.  --tracks-bedgraph: also the number of colours per interval as" << std::endl
			<< "               bedGraph.  Combines with all tables above (the same colours).  One GPU only." << std::endl
			<< "       --variants: also write the alleles the genomes walk through the superbubbles as TSV to --variants-out (default" << std::endl
			<< "               de_bruijn.variants.tsv): every sequence walked through every superbubble (--superbubbles-max) on both strands, the walks" << std::endl
			<< "               that read the same inside sides are one allele: site, entrance, exit, allele, traversals, sides, edges, number of colours," << std::endl
			<< "               presence bits, the span of its first traversal and whether it is the reference's.  --variants-ref: the reference colour." << std::endl
			<< "               --variants-vcf: with a reference, also VCF 4.2 on the reference's coordinates, one sample per colour, not normalised." << std::endl
			<< "               Combines with all tables above (the same colours); written last.  One GPU only." << std::endl;
	}
}

namespace
{
	// TWOPACO_TIMING=1: milliseconds since the process was started (exec), from /proc/self/stat
	double SinceProcessStart()
	{
		std::FILE * f = std::fopen("/proc/self/stat", "r");
		if (!f) return -1;
		char buf[2048];
		size_t n = std::fread(buf, 1, sizeof(buf) - 1, f);
		std::fclose(f);
		buf[n] = 0;
		const char * p = std::strrchr(buf, ')');
		if (!p) return -1;
		unsigned long long start = 0;
		int field = 2;
		for (p++; *p && field < 22; p++) if (*p == ' ') { field++; if (field == 22) { start = std::strtoull(p + 1, 0, 10); break; } }
		struct timespec ts;
		clock_gettime(CLOCK_BOOTTIME, &ts);
		const double now = ts.tv_sec * 1e3 + ts.tv_nsec / 1e6;
		return now - double(start) * 1e3 / double(sysconf(_SC_CLK_TCK));
	}
}

int main(int argc, char * argv[])
{
	const bool timing = std::getenv("TWOPACO_TIMING") != 0;
	if (timing) std::cerr << "[timing] exec -> main: " << SinceProcessStart() << " ms" << std::endl;
	try
	{
		unsigned int kvalue = 25, hashFunctions = 5, rounds = 1, threads = 1;
		size_t abundance = UINT64_MAX;
		bool filterSizeSet = false, filterMemorySet = false, runTests = false, roundsSet = false;
		unsigned int filterSize = 32;
		double filterMemory = 4;
		std::string tmpDirName = ".", outFileName = "de_bruijn.bin";
		std::vector<std::string> fileName;
		TwoPaCo::EnumeratorOptions options;
		TwoPaCo::GraphFormat::TableOptions tables;
		bool optionsSet = false, outFileSet = false, graphOutSet = false, graphTextSet = false;
		for (int i = 1; i < argc; i++)
		{
			std::string a = argv[i];
			auto value = [&](const std::string & argId) -> std::string
			{
				if (i + 1 >= argc) throw ArgError("Missing a value for this argument!", argId);
				return argv[++i];
			};

			if (Match(a, "k", "kvalue"))
			{
				kvalue = Parse<unsigned int>(value("(--kvalue)"), "(--kvalue)");
				if (kvalue % 2 != 1) throw ArgError("Value '" + std::to_string(kvalue) + "' does not meet constraint: value of K must be odd", "(--kvalue)");
			}
			else if (Match(a, "f", "filtersize"))
			{
				const std::string v = value("(--filtersize)");
				if (v == "auto") options.autoFilterSize = true; else filterSize = Parse<unsigned int>(v, "(--filtersize)");
				filterSizeSet = true;
			}
			else if (Match(a, 0, "filtermemory")) { filterMemory = std::atof(value("(--filtermemory)").c_str()); filterMemorySet = true; }
			else if (Match(a, "q", "hashfnumber")) hashFunctions = Parse<unsigned int>(value("(--hashfnumber)"), "(--hashfnumber)");
			else if (Match(a, "r", "rounds")) { rounds = Parse<unsigned int>(value("(--rounds)"), "(--rounds)"); roundsSet = true; }
			else if (Match(a, "t", "threads")) threads = Parse<unsigned int>(value("(--threads)"), "(--threads)");
			else if (Match(a, "a", "abundance")) abundance = Parse<size_t>(value("(--abundance)"), "(--abundance)");
			else if (Match(a, 0, "tmpdir")) tmpDirName = value("(--tmpdir)");
			else if (Match(a, "o", "outfile")) { outFileName = value("(--outfile)"); outFileSet = true; }
			else if (Match(a, 0, "test")) runTests = true;
			else if (Match(a, 0, "seed")) { options.pinnedSeed = true; options.seed = Parse<uint64_t>(value("(--seed)"), "(--seed)"); optionsSet = true; }
			else if (Match(a, 0, "device")) { options.device = int(Parse<unsigned int>(value("(--device)"), "(--device)")); optionsSet = true; }
			else if (Match(a, 0, "test-first")) { options.insertTestFirst = true; optionsSet = true; }
			else if (Match(a, 0, "gpus")) { options.gpus = int(Parse<unsigned int>(value("(--gpus)"), "(--gpus)")); optionsSet = true; }
			else if (Match(a, 0, "no-rccl")) { options.rccl = false; optionsSet = true; }
			else if (Match(a, 0, "emulate-ranks")) { options.emulateRanks = true; optionsSet = true; }
			else if (Match(a, 0, "save-filter")) { options.saveFilter = value("(--save-filter)"); optionsSet = true; }
			else if (Match(a, 0, "load-filter")) { options.loadFilter = value("(--load-filter)"); optionsSet = true; }
			else if (Match(a, 0, "graph"))
			{
				options.graphFormat = value("(--graph)");
				if (options.graphFormat != "gfa1" && options.graphFormat != "gfa2" && options.graphFormat != "fasta")
				{
					throw ArgError("Value '" + options.graphFormat + "' does not meet constraint: gfa1|gfa2|fasta", "(--graph)");
				}

				optionsSet = true;
			}
			else if (Match(a, 0, "graph-out")) { options.graphFile = value("(--graph-out)"); graphOutSet = true; }
			else if (Match(a, 0, "graph-prefix")) options.graphPrefix = true;
			else if (Match(a, 0, "graph-threads"))
			{
				const std::string v = value("(--graph-threads)");
				char * end = 0;
				const long long parsed = std::strtoll(v.c_str(), &end, 10);
				if (end == v.c_str() || *end != 0 || parsed < 1) throw ArgError("Couldn't read argument value from string '" + v + "'", "(--graph-threads)");
				options.graphThreads = size_t(std::min<long long>(parsed, 16));
			}
			else if (Match(a, 0, "graph-text"))
			{
				const std::string v = value("(--graph-text)");
				if (v != "host" && v != "device") throw ArgError("Value '" + v + "' does not meet constraint: host|device", "(--graph-text)");
				options.graphTextOnDevice = v == "device";
				graphTextSet = true;
			}
			else if (Match(a, 0, "graph-compact")) { options.graphCompact = true; optionsSet = true; }
			else if (TwoPaCo::GraphFormat::ParseTableOption(a, value, "", tables)) continue;
			else if (Match(a, "h", "help")) { Usage(); return 0; }
			else if (a == "--version") { std::cout << argv[0] << "  version: 1.1.0" << std::endl; return 0; }
			else if (a.size() > 1 && a[0] == '-') throw ArgError("Couldn't find match for argument", "(" + a + ")");
			else fileName.push_back(a);
		}

		if (filterSizeSet == filterMemorySet)
		{
			throw ArgError(filterSizeSet ? "Mutually exclusive argument already set!" : "One of the required arguments is missing!", "(--filtersize|--filtermemory)");
		}

		if (fileName.empty())
		{
			throw ArgError("Required argument missing: filenames", "(filenames)");
		}

		if (options.autoFilterSize)
		{
			if (options.gpus > 1) throw ArgError("The filter size is chosen on one GPU only (every rank holds a chunk of the text, and their sketches are not merged): not with --gpus above 1", "(--filtersize)");
			if (!options.loadFilter.empty()) throw ArgError("A Bloom filter checkpoint fixes the filter size: not with --load-filter", "(--filtersize)");
			if (runTests) throw ArgError("The self-test draws its own filter sizes: not with --test", "(--filtersize)");
			options.autoRounds = !roundsSet;
			optionsSet = true;
		}

		if (options.graphCompact)
		{
			if (options.graphFormat != "gfa1") throw ArgError("The compact graph is gfa1 with every link once: it needs --graph gfa1", "(--graph-compact)");
			if (options.graphTextOnDevice) throw ArgError("The compact graph is formatted by the host: not with --graph-text device", "(--graph-compact)");
			if (options.gpus > 1) throw ArgError("The compact graph is written by one GPU only (every rank holds its own piece of the junction stream): not with --gpus above 1", "(--graph-compact)");
		}

		if (!options.graphFormat.empty())
		{
			if (options.gpus > 1) throw ArgError("The graph is written by one GPU only (every rank holds its own piece of the junction stream): not with --gpus above 1", "(--graph)");
			if (!graphOutSet) options.graphFile = "de_bruijn." + options.graphFormat;
			if (!outFileSet) outFileName.clear();  // the junction stream stays on the device
		}
		else if (graphOutSet || options.graphPrefix || graphTextSet)
		{
			throw ArgError("This argument needs --graph <gfa1|gfa2|fasta>", graphOutSet ? "(--graph-out)" : options.graphPrefix ? "(--graph-prefix)" : "(--graph-text)");
		}

		// every table beside every other, each into a file of its own, on one GPU; the complaints are looked for in the tables' order
		namespace GF = TwoPaCo::GraphFormat;
		const GF::TableCliRules rules = {"", {GF::COLORS, GF::LINKS, GF::BUBBLES, GF::DISTANCES, GF::COMPONENTS, GF::SUPERBUBBLES, GF::ANCHORS, GF::LOCATE, GF::CLASSES, GF::TRACKS, GF::VARIANTS}, false, false, false, false,
			{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {false, false, false, false, false, false, false, false, false, false, false}, options.gpus, true, fileName.size()};
		GF::CheckTableOptions(tables, rules);
		options.tables = tables.request;
		optionsSet = optionsSet || options.tables.Any();

		if (runTests)
		{
			size_t trials = 10;
			if (const char * t = std::getenv("TWOPACO_SELFTEST_TRIALS")) trials = size_t(std::atoi(t));
			// reference constructor.cpp:164 runs the trials off std::random_device; --seed makes them (and a failure) reproducible
			if (options.pinnedSeed)
			{
				return TwoPaCo::RunTestsSeeded(options.seed, trials, 20, 9000, 6, TwoPaCo::Range(3, 11), TwoPaCo::Range(1, 2), TwoPaCo::Range(1, 5), TwoPaCo::Range(4, 5), 0.05, 0.1, tmpDirName) ? 0 : 1;
			}

			return TwoPaCo::RunTests(trials, 20, 9000, 6, TwoPaCo::Range(3, 11), TwoPaCo::Range(1, 2), TwoPaCo::Range(1, 5), TwoPaCo::Range(4, 5), 0.05, 0.1, tmpDirName) ? 0 : 1;
		}

		int64_t filterBits = filterSizeSet ? int64_t(filterSize) : int64_t(std::log2(filterMemory * 8e+9));
		std::unique_ptr<TwoPaCo::VertexEnumerator> vid = optionsSet
			? TwoPaCo::CreateEnumerator(fileName, kvalue, size_t(filterBits), hashFunctions, rounds, threads, abundance, tmpDirName, outFileName, std::cout, options)
			: TwoPaCo::CreateEnumerator(fileName, kvalue, size_t(filterBits), hashFunctions, rounds, threads, abundance, tmpDirName, outFileName, std::cout);
		if (vid)
		{
			std::cout << "Distinct junctions = " << vid->GetVerticesCount() << std::endl;
			std::cout << std::endl;
		}

		if (timing) std::cerr << "[timing] exec -> output complete: " << SinceProcessStart() << " ms" << std::endl;
		// Device memory is released here, explicitly (a few ms).  What is left of a normal exit is the HIP runtime's own
		// teardown (code objects, queues: ~0.1 s for nothing the process still needs), so the process ends right after
		// flushing its streams unless TWOPACO_CLEAN_EXIT is set.
		vid.reset();
		if (timing) std::cerr << "[timing] exec -> context destroyed: " << SinceProcessStart() << " ms" << std::endl;
		if (!std::getenv("TWOPACO_CLEAN_EXIT"))
		{
			std::cout.flush();
			std::cerr.flush();
			std::fflush(0);
			std::_Exit(0);
		}
	}
	catch (ArgError & e)
	{
		std::cerr << std::endl << "Error: " << e.what() << " for arg " << e.arg << std::endl;
		return 1;
	}
	catch (std::runtime_error & e)
	{
		std::cerr << std::endl << "Error: " << e.what() << std::endl;
		return 1;
	}

	return 0;
}
