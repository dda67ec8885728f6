// devicegraph.h -- the tables of the compacted graph, built on the device (include/twopaco_hip.h, the tpc_segments_* groups) and
// fetched into the structs of graphformat.h.  One layer for both programs: graphdump, which loads the device library with dlopen,
// and twopaco, which links it.  What differs between them stays with them: their timers, their [timing] lines (StageObserver), the
// text they throw when an entry point fails (Api::check is the caller's) or a stage disagrees with them (StageWording), the order of
// their stages, and when they fetch the event table.  Nothing here knows which program calls it.
#ifndef _DEVICE_GRAPH_H_
#define _DEVICE_GRAPH_H_

#include <algorithm>
#include <functional>
#include <stdexcept>
#include <vector>

#include "../../include/twopaco_hip.h"
#include "graphformat.h"
#include "tablerequest.h"
#include "textpack.h"

// The entry points both programs reach through Api, each as tpc_<name>: the one list behind the members, graphdump's dlsym loads
// (Api::Load) and twopaco's direct addresses (filled where the symbols are linked: vertexenumerator.cpp).
#define TPC_DEVICE_GRAPH_ENTRY_POINTS(X) \
	X(ctx_create) X(ctx_destroy) X(last_error) X(seq_upload) X(kernel_ms) \
	X(segments_build_host) X(segments_counts) X(segments_error) \
	X(segments_fetch_names) X(segments_fetch_first) X(segments_fetch_events) X(segments_fetch_sequences) \
	X(segments_text_plan) X(segments_text_write) \
	X(segments_colors_build) X(segments_colors_fetch_rows) X(segments_colors_fetch_presence) X(segments_colors_fetch_hist) \
	X(segments_links_build) X(segments_links_info) X(segments_links_fetch_rows) X(segments_links_fetch_first) \
	X(segments_bubbles_build) X(segments_bubbles_info) X(segments_bubbles_fetch_rows) X(segments_bubbles_fetch_hist) \
	X(segments_distances_build) X(segments_distances_info) X(segments_distances_fetch) \
	X(segments_components_build) X(segments_components_info) X(segments_components_fetch_members) X(segments_components_fetch_rows) \
	X(segments_components_fetch_presence) \
	X(segments_superbubbles_build) X(segments_superbubbles_info) X(segments_superbubbles_fetch_rows) X(segments_superbubbles_fetch_members) \
	X(segments_superbubbles_fetch_presence) \
	X(segments_anchors_build) X(segments_anchors_info) X(segments_anchors_fetch_mates) X(segments_anchors_fetch_rows) X(segments_anchors_fetch_shared) \
	X(segments_edges_build) X(segments_edges_info) X(segments_locate) X(segments_locate_info) X(segments_locate_fetch_runs) X(segments_locate_fetch_records) \
	X(segments_locate_fetch_shared) \
	X(segments_classes_build) X(segments_classes_info) X(segments_classes_fetch_members) X(segments_classes_fetch_rows) X(segments_classes_fetch_presence) \
	X(segments_tracks_build) X(segments_tracks_info) X(segments_tracks_fetch_rows) X(segments_tracks_fetch_colors) X(segments_tracks_fetch_depth) \
	X(segments_variants_build) X(segments_variants_info) X(segments_variants_fetch_traversals) X(segments_variants_fetch_alleles) X(segments_variants_fetch_presence) \
	X(segments_variants_fetch_sites)

namespace TwoPaCo
{
	// (hidden: every program compiles its own copy, libtwopaco_host.so exports none of it)
	namespace DeviceGraph __attribute__((visibility("hidden")))
	{
		struct Api
		{
#define X(name) decltype(&tpc_##name) name;
			TPC_DEVICE_GRAPH_ENTRY_POINTS(X)
#undef X
			tpc_ctx * ctx;
			// the caller's: throws its own text when rc != 0.  what: the entry point without its tpc_
			std::function<void(int rc, const char * what)> check;

			Api() : ctx(0) {}

			// every entry point from find("tpc_<name>"), which returns its address or throws
			template<class Find> void Load(Find find)
			{
#define X(name) name = reinterpret_cast<decltype(name)>(find("tpc_" #name));
				TPC_DEVICE_GRAPH_ENTRY_POINTS(X)
#undef X
			}
		};

		// The event table of the last segment build as far as it was fetched: `table` points into the arrays.
		struct Events
		{
			std::vector<int64_t> name;
			std::vector<uint32_t> first, begin, end, seqEventBegin;
			GraphFormat::EventTable table;

			// seqEventBegin is all zeros until FetchSequences
			Events(uint64_t events, size_t sequences) : seqEventBegin(sequences + 1, 0)
			{
				table.events = events;
				table.sequences = sequences;
				table.seqEventBegin = seqEventBegin.data();
			}
		};

		inline void FetchNames(const Api & api, Events & held)
		{
			held.name.resize(held.table.events);
			api.check(api.segments_fetch_names(api.ctx, 0, held.table.events, held.name.data()), "segments_fetch_names");
			held.table.name = held.name.data();
		}

		inline void FetchFirst(const Api & api, Events & held)
		{
			held.first.resize((held.table.events + 31) / 32);
			api.check(api.segments_fetch_first(api.ctx, 0, held.first.size(), held.first.data()), "segments_fetch_first");
			held.table.first = held.first.data();
		}

		inline void FetchPositions(const Api & api, Events & held)
		{
			held.begin.resize(held.table.events);
			held.end.resize(held.table.events);
			api.check(api.segments_fetch_events(api.ctx, 0, held.table.events, held.begin.data(), held.end.data()), "segments_fetch_events");
			held.table.begin = held.begin.data();
			held.table.end = held.end.data();
		}

		inline void FetchSequences(const Api & api, Events & held)
		{
			api.check(api.segments_fetch_sequences(api.ctx, 0, held.seqEventBegin.size(), held.seqEventBegin.data()), "segments_fetch_sequences");
		}

		// The colour table (csrc/tpc_colors.hip): the events of the table on the device grouped by segment there.
		inline void BuildColors(const Api & api, const GraphFormat::ColorMap & map)
		{
			api.check(api.segments_colors_build(api.ctx, map.colorOfSequence.data(), uint32_t(map.label.size())), "segments_colors_build");
		}

		// ... fetched: the rows, their presence words and the histogram
		inline void FetchColors(const Api & api, const GraphFormat::ColorMap & map, uint64_t rows, GraphFormat::ColorTable & out)
		{
			out.colors = map.label.size();
			out.firstEvent.resize(rows);
			out.occurrences.resize(rows);
			out.forward.resize(rows);
			out.nColors.resize(rows);
			out.presence.resize(rows * out.Words());
			out.histSegments.resize(out.colors + 1);
			out.histBases.resize(out.colors + 1);
			api.check(api.segments_colors_fetch_rows(api.ctx, 0, rows, out.firstEvent.data(), out.occurrences.data(), out.forward.data(), out.nColors.data()), "segments_colors_fetch_rows");
			api.check(api.segments_colors_fetch_presence(api.ctx, 0, rows, out.presence.data()), "segments_colors_fetch_presence");
			api.check(api.segments_colors_fetch_hist(api.ctx, out.histSegments.data(), out.histBases.data()), "segments_colors_fetch_hist");
		}

		// The link table (csrc/tpc_links.hip): the distinct links of the table on the device found there.
		inline void BuildLinks(const Api & api)
		{
			api.check(api.segments_links_build(api.ctx), "segments_links_build");
		}

		// ... fetched: the rows (for the link file and the bubbles' header) and / or the first bits (for the compact text, never an
		// empty array).  Returns the number of rows, fetched or not.
		inline uint64_t FetchLinks(const Api & api, uint64_t events, bool rows, bool bits, GraphFormat::LinkTable & out)
		{
			uint64_t info[4] = {0, 0, 0, 0};
			api.check(api.segments_links_info(api.ctx, info), "segments_links_info");
			out.occurrences = info[1];
			if (rows)
			{
				out.firstEvent.resize(info[0]);
				out.count.resize(info[0]);
				out.same.resize(info[0]);
				api.check(api.segments_links_fetch_rows(api.ctx, 0, info[0], out.firstEvent.data(), out.count.data(), out.same.data()), "segments_links_fetch_rows");
			}

			if (bits)
			{
				out.linkFirst.assign(std::max<size_t>(1, size_t((events + 31) / 32)), 0);
				api.check(api.segments_links_fetch_first(api.ctx, 0, (events + 31) / 32, out.linkFirst.data()), "segments_links_fetch_first");
			}

			return info[0];
		}

		// The simple bubbles (csrc/tpc_bubbles.hip), found over the link rows where they lie.
		inline void BuildBubbles(const Api & api)
		{
			api.check(api.segments_bubbles_build(api.ctx), "segments_bubbles_build");
		}

		// ... fetched: the bubble rows and the degree histogram
		inline void FetchBubbles(const Api & api, GraphFormat::BubbleTable & out)
		{
			uint64_t info[4] = {0, 0, 0, 0};
			api.check(api.segments_bubbles_info(api.ctx, info), "segments_bubbles_info");
			out.sides = info[1];
			out.arcs = info[2];
			out.source.resize(info[0]);
			out.armA.resize(info[0]);
			out.armB.resize(info[0]);
			out.sink.resize(info[0]);
			api.check(api.segments_bubbles_fetch_rows(api.ctx, 0, info[0], out.source.data(), out.armA.data(), out.armB.data(), out.sink.data()), "segments_bubbles_fetch_rows");
			api.check(api.segments_bubbles_fetch_hist(api.ctx, out.hist), "segments_bubbles_fetch_hist");
		}

		// The distance matrices (csrc/tpc_distances.hip), summed over the presence bits of the colour build where they lie.
		inline void BuildDistances(const Api & api)
		{
			api.check(api.segments_distances_build(api.ctx), "segments_distances_build");
		}

		// ... fetched: the two matrices.  false, and nothing fetched, when the stage saw other colours or segments than the caller
		inline bool FetchDistances(const Api & api, uint64_t colors, uint64_t rows, GraphFormat::DistanceTable & out)
		{
			uint64_t info[4] = {0, 0, 0, 0};
			api.check(api.segments_distances_info(api.ctx, info), "segments_distances_info");
			if (info[0] != colors || info[1] != rows) return false;
			out.colors = info[0];
			out.segments.resize(size_t(info[0] * info[0]));
			out.edges.resize(size_t(info[0] * info[0]));
			api.check(api.segments_distances_fetch(api.ctx, 0, info[0], out.segments.data(), out.edges.data()), "segments_distances_fetch");
			return true;
		}

		// The connected components (csrc/tpc_components.hip), found over the link rows and summed over the colour rows where they lie.
		inline void BuildComponents(const Api & api)
		{
			api.check(api.segments_components_build(api.ctx), "segments_components_build");
		}

		// ... fetched: the members, the rows and their presence words.  false, and nothing fetched, when the stage saw other segments
		// than the caller
		inline bool FetchComponents(const Api & api, uint64_t rows, size_t words, GraphFormat::ComponentTable & out)
		{
			uint64_t info[4] = {0, 0, 0, 0};
			api.check(api.segments_components_info(api.ctx, info), "segments_components_info");
			if (info[1] != rows) return false;
			const size_t n = size_t(info[0]);
			out.component.resize(rows);
			out.root.resize(n);
			out.segments.resize(n);
			out.links.resize(n);
			out.length.resize(n);
			out.edges.resize(n);
			out.occurrences.resize(n);
			out.presence.resize(n * words);
			api.check(api.segments_components_fetch_members(api.ctx, 0, rows, out.component.data()), "segments_components_fetch_members");
			api.check(api.segments_components_fetch_rows(api.ctx, 0, n, out.root.data(), out.segments.data(), out.links.data(), out.length.data(), out.edges.data(),
				out.occurrences.data()), "segments_components_fetch_rows");
			api.check(api.segments_components_fetch_presence(api.ctx, 0, n, out.presence.data()), "segments_components_fetch_presence");
			return true;
		}

		// The colour classes (csrc/tpc_classes.hip), grouped over the presence words of the colour build where they lie.
		inline void BuildClasses(const Api & api)
		{
			api.check(api.segments_classes_build(api.ctx), "segments_classes_build");
		}

		// ... fetched: the members, the rows and their presence words (the per-n sets are the writer's to sum).  false, and nothing
		// fetched, when the stage saw other segments than the caller
		inline bool FetchClasses(const Api & api, uint64_t rows, size_t words, GraphFormat::ClassTable & out)
		{
			uint64_t info[5] = {0, 0, 0, 0, 0};
			api.check(api.segments_classes_info(api.ctx, info), "segments_classes_info");
			if (info[1] != rows) return false;
			const size_t n = size_t(info[0]);
			out.classOf.resize(rows);
			out.first.resize(n);
			out.segments.resize(n);
			out.length.resize(n);
			out.edges.resize(n);
			out.occurrences.resize(n);
			out.presence.resize(n * words);
			api.check(api.segments_classes_fetch_members(api.ctx, 0, rows, out.classOf.data()), "segments_classes_fetch_members");
			api.check(api.segments_classes_fetch_rows(api.ctx, 0, n, out.first.data(), out.segments.data(), out.length.data(), out.edges.data(), out.occurrences.data()),
				"segments_classes_fetch_rows");
			api.check(api.segments_classes_fetch_presence(api.ctx, 0, n, out.presence.data()), "segments_classes_fetch_presence");
			return true;
		}

		// The presence tracks (csrc/tpc_tracks.hip): the colour rows of the colour build projected onto the events of the table on the device.
		inline void BuildTracks(const Api & api, const GraphFormat::ColorMap & map, uint32_t only)
		{
			api.check(api.segments_tracks_build(api.ctx, map.colorOfSequence.data(), uint32_t(map.label.size()), only), "segments_tracks_build");
		}

		// ... fetched: the intervals and the sums.  false, and nothing fetched, when the stage saw other colours than the caller
		inline bool FetchTracks(const Api & api, const GraphFormat::ColorMap & map, uint64_t segments, GraphFormat::TrackTable & out)
		{
			uint64_t info[5] = {0, 0, 0, 0, 0};
			api.check(api.segments_tracks_info(api.ctx, info), "segments_tracks_info");
			if (info[2] != map.label.size()) return false;
			const size_t n = size_t(info[0]);
			out.colors = info[2];
			out.only = uint32_t(info[3]);
			out.segments = segments;
			out.firstEvent.resize(n);
			out.lastEvent.resize(n);
			out.row.resize(n);
			out.intervals.resize(size_t(out.colors));
			out.edges.resize(size_t(out.colors));
			out.coreEdges.resize(size_t(out.colors));
			out.privateEdges.resize(size_t(out.colors));
			out.depthIntervals.resize(size_t(out.colors) + 1);
			out.depthEdges.resize(size_t(out.colors) + 1);
			api.check(api.segments_tracks_fetch_rows(api.ctx, 0, n, out.firstEvent.data(), out.lastEvent.data(), out.row.data()), "segments_tracks_fetch_rows");
			api.check(api.segments_tracks_fetch_colors(api.ctx, out.intervals.data(), out.edges.data(), out.coreEdges.data(), out.privateEdges.data()), "segments_tracks_fetch_colors");
			api.check(api.segments_tracks_fetch_depth(api.ctx, out.depthIntervals.data(), out.depthEdges.data()), "segments_tracks_fetch_depth");
			return true;
		}

		// The variants (csrc/tpc_variants.hip): every sequence walked through the superbubbles of the superbubble build on the device.
		inline void BuildVariants(const Api & api, const GraphFormat::ColorMap & map, uint32_t ref)
		{
			api.check(api.segments_variants_build(api.ctx, map.colorOfSequence.data(), uint32_t(map.label.size()), ref), "segments_variants_build");
		}

		// ... fetched: the traversals, the alleles with their presence words and the sites.  false, and nothing fetched, when the stage
		// saw other colours or superbubbles than the caller
		inline bool FetchVariants(const Api & api, const GraphFormat::ColorMap & map, uint64_t segments, size_t superbubbles, GraphFormat::VariantTable & out)
		{
			uint64_t info[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
			api.check(api.segments_variants_info(api.ctx, info), "segments_variants_info");
			if (info[5] != map.label.size() || info[8] != superbubbles) return false;
			const size_t alleles = size_t(info[1]), n = size_t(info[2]), words = size_t((info[5] + 31) / 32);
			out.colors = info[5];
			out.segments = segments;
			out.strays = info[3];
			out.ref = uint32_t(info[6]);
			for (std::vector<uint32_t> * v : {&out.start, &out.last, &out.dir, &out.row, &out.edges}) v->resize(n);
			out.mask.resize(n);
			for (std::vector<uint32_t> * v : {&out.alleleRow, &out.sides, &out.alleleEdges, &out.first, &out.nColors}) v->resize(alleles);
			out.alleleMask.resize(alleles);
			out.traversals.resize(alleles);
			out.presence.resize(alleles * words);
			out.alleleOffset.resize(superbubbles + 1);
			out.refAllele.resize(superbubbles);
			out.siteTraversals.resize(superbubbles);
			out.refTraversals.resize(superbubbles);
			api.check(api.segments_variants_fetch_traversals(api.ctx, 0, n, out.start.data(), out.last.data(), out.dir.data(), out.row.data(), out.edges.data(), out.mask.data()),
				"segments_variants_fetch_traversals");
			api.check(api.segments_variants_fetch_alleles(api.ctx, 0, alleles, out.alleleRow.data(), out.sides.data(), out.alleleEdges.data(), out.first.data(), out.nColors.data(),
				out.alleleMask.data(), out.traversals.data()), "segments_variants_fetch_alleles");
			api.check(api.segments_variants_fetch_presence(api.ctx, 0, alleles, out.presence.data()), "segments_variants_fetch_presence");
			api.check(api.segments_variants_fetch_sites(api.ctx, 0, superbubbles, out.alleleOffset.data(), out.siteTraversals.data(), out.refAllele.data(), out.refTraversals.data()),
				"segments_variants_fetch_sites");
			return true;
		}

		// The bounded superbubbles (csrc/tpc_superbubbles.hip), searched over the link rows' arcs, presence ORed over the colour rows.
		inline void BuildSuperbubbles(const Api & api, uint32_t maxInside)
		{
			api.check(api.segments_superbubbles_build(api.ctx, maxInside), "segments_superbubbles_build");
		}

		// ... fetched: the rows, their members and presence words; the adjacency and exit[] stay on the device.  false, and nothing
		// fetched, when the stage saw other segments than the caller
		inline bool FetchSuperbubbles(const Api & api, uint64_t rows, size_t words, GraphFormat::SuperbubbleTable & out)
		{
			uint64_t info[7] = {0, 0, 0, 0, 0, 0, 0};
			api.check(api.segments_superbubbles_info(api.ctx, info), "segments_superbubbles_info");
			if (info[1] != 2 * rows) return false;
			const size_t n = size_t(info[0]);
			out.sides = info[1];
			out.unmirrored = info[3];
			out.arcs = info[5];
			out.maxInside = uint32_t(info[6]);
			out.entrance.resize(n);
			out.exit.resize(n);
			out.inside.resize(n);
			out.arcsIn.resize(n);
			out.nColors.resize(n);
			out.paths.resize(n);
			out.minEdges.resize(n);
			out.maxEdges.resize(n);
			out.presence.resize(n * words);
			out.memberOffset.resize(n + 1);
			out.members.resize(size_t(info[2]));
			api.check(api.segments_superbubbles_fetch_rows(api.ctx, 0, n, out.entrance.data(), out.exit.data(), out.inside.data(), out.arcsIn.data(), out.nColors.data(),
				out.paths.data(), out.minEdges.data(), out.maxEdges.data()), "segments_superbubbles_fetch_rows");
			api.check(api.segments_superbubbles_fetch_members(api.ctx, out.memberOffset.data(), out.members.data()), "segments_superbubbles_fetch_members");
			api.check(api.segments_superbubbles_fetch_presence(api.ctx, 0, n, out.presence.data()), "segments_superbubbles_fetch_presence");
			return true;
		}

		// The anchor blocks (csrc/tpc_anchors.hip): the events of the table on the device paired with the reference colour's and chained there.
		inline void BuildAnchors(const Api & api, const GraphFormat::ColorMap & map, uint32_t ref)
		{
			api.check(api.segments_anchors_build(api.ctx, map.colorOfSequence.data(), uint32_t(map.label.size()), ref), "segments_anchors_build");
		}

		// ... fetched: the mates, the blocks and the per-colour sums.  false, and nothing fetched, when the stage saw other colours than
		// the caller
		inline bool FetchAnchors(const Api & api, const GraphFormat::ColorMap & map, uint64_t events, uint64_t segments, GraphFormat::AnchorTable & out)
		{
			uint64_t info[6] = {0, 0, 0, 0, 0, 0};
			api.check(api.segments_anchors_info(api.ctx, info), "segments_anchors_info");
			if (info[2] != map.label.size()) return false;
			const size_t n = size_t(info[0]);
			out.colors = info[2];
			out.ref = uint32_t(info[3]);
			out.refEdges = info[4];
			out.segments = segments;
			out.mate.resize(size_t(events));
			out.queryFirst.resize(n);
			out.queryLast.resize(n);
			out.refFirst.resize(n);
			out.refLast.resize(n);
			out.blocks.resize(size_t(out.colors));
			out.anchors.resize(size_t(out.colors));
			out.edges.resize(size_t(out.colors));
			out.reverseEdges.resize(size_t(out.colors));
			api.check(api.segments_anchors_fetch_mates(api.ctx, 0, events, out.mate.data()), "segments_anchors_fetch_mates");
			api.check(api.segments_anchors_fetch_rows(api.ctx, 0, n, out.queryFirst.data(), out.queryLast.data(), out.refFirst.data(), out.refLast.data()), "segments_anchors_fetch_rows");
			api.check(api.segments_anchors_fetch_shared(api.ctx, out.blocks.data(), out.anchors.data(), out.edges.data(), out.reverseEdges.data()), "segments_anchors_fetch_shared");
			return true;
		}

		// The edge index over the table and the text on the device (csrc/tpc_locate.hip); info: tpc_segments_edges_info
		inline void BuildEdges(const Api & api, uint64_t * info)
		{
			api.check(api.segments_edges_build(api.ctx), "segments_edges_build");
			api.check(api.segments_edges_info(api.ctx, info), "segments_edges_info");
		}

		// The query records through the edge index in BATCHES of whole records of at most batchPositions positions of packed text (a
		// longer record is a batch of its own): the sums are per record and the runs ascend, so the batches only concatenate.  The
		// colour table on the device at the time must be the caller's (`colors` colours).  edges: what BuildEdges reported; kernelMs:
		// TPC_K_LOCATE summed over the batches.  Returns the number of batches.
		inline uint64_t LocateOnDevice(const Api & api, const uint64_t * edges, uint64_t colors, uint64_t segments, const GraphFormat::LoadedSequences & queries, uint64_t batchPositions,
			GraphFormat::LocateTable & out, double & kernelMs)
		{
			kernelMs = 0;
			uint64_t info[6] = {0, 0, 0, 0, 0, 0};
			out = GraphFormat::LocateTable();
			out.colors = colors;
			out.segments = segments;
			out.entries = edges[0];
			out.duplicates = edges[1];
			const size_t records = queries.body.size();
			out.windows.assign(records, 0);
			out.found.assign(records, 0);
			out.forward.assign(records, 0);
			out.runs.assign(records, 0);
			out.shared.assign(records * size_t(colors), 0);
			std::vector<uint8_t> codes;
			uint64_t batches = 0;
			for (size_t first = 0; first < records; ++batches)
			{
				TwoPaCo::PackedText text;
				text.BeginText();
				size_t last = first;
				while (last < records && (last == first || text.length + queries.body[last].size() + 1 <= batchPositions))
				{
					const std::string & body = queries.body[last];
					codes.resize(body.size());
					for (size_t i = 0; i < body.size(); i++) codes[i] = body[i] == 'A' ? 0 : body[i] == 'C' ? 1 : body[i] == 'G' ? 2 : body[i] == 'T' ? 3 : 4;
					text.AppendCodes(codes.data(), codes.size());
					text.EndRecord(codes.size());
					++last;
				}

				const size_t n = last - first;
				api.check(api.segments_locate(api.ctx, text.bases.data(), text.nmask.data(), text.length, text.recStart.data(), text.recLength.data(), uint32_t(n)), "segments_locate");
				kernelMs += api.kernel_ms(api.ctx, TPC_K_LOCATE);
				api.check(api.segments_locate_info(api.ctx, info), "segments_locate_info");
				if (info[4] != colors) throw std::runtime_error("the locate stage and the colour map disagree about the colours");
				api.check(api.segments_locate_fetch_records(api.ctx, 0, n, &out.windows[first], &out.found[first], &out.forward[first], &out.runs[first]), "segments_locate_fetch_records");
				if (colors) api.check(api.segments_locate_fetch_shared(api.ctx, 0, n, &out.shared[first * size_t(colors)]), "segments_locate_fetch_shared");
				const size_t runs = size_t(info[3]), at = out.Runs();
				std::vector<uint32_t> qFirst(runs);
				out.runLength.resize(at + runs);
				out.runRow.resize(at + runs);
				out.runRev.resize(at + runs);
				out.runOff.resize(at + runs);
				api.check(api.segments_locate_fetch_runs(api.ctx, 0, runs, qFirst.data(), out.runLength.data() + at, out.runRow.data() + at, out.runRev.data() + at, out.runOff.data() + at),
					"segments_locate_fetch_runs");
				for (size_t i = 0; i < runs; i++)
				{
					// the record of a run: the last one that starts at or before its first window
					const size_t r = size_t(std::upper_bound(text.recStart.begin(), text.recStart.end(), uint64_t(qFirst[i])) - text.recStart.begin());
					if (r == 0 || r > n) throw std::runtime_error("the locate stage reports a run outside the query records");
					out.runQuery.push_back(first + r - 1);
					out.runBegin.push_back(qFirst[i] - text.recStart[r - 1]);
				}

				first = last;
			}

			return batches;
		}

		// Where a position of a record is ambiguous, in the packed text's coordinates: what the segment build must not name by.
		// refusal: thrown when the packed text and the parsed letters are not the same records
		inline std::vector<uint64_t> AmbiguousPositions(const TwoPaCo::PackedText & text, const GraphFormat::LoadedSequences & loaded, const char * refusal)
		{
			if (text.recStart.size() != loaded.body.size()) throw std::runtime_error(refusal);
			std::vector<uint64_t> ambiguous;
			for (size_t r = 0; r < loaded.body.size(); r++)
			{
				if (text.recLength[r] != loaded.body[r].size()) throw std::runtime_error(refusal);
				for (uint64_t at : loaded.ambiguous[r]) ambiguous.push_back(text.recStart[r] + at);
			}

			return ambiguous;
		}

		// The stages of BuildTables: one per table (GraphFormat::TableId), and the edge index in front of the locate stage
		const int EDGES = GraphFormat::TABLES;
		// twopaco's order, and graphdump's: the distance stage before the link stage, as long as graphdump has had both.  Behind the link
		// and the bubble stage it would find 12 B per link, 4 B per 32 events and, with --bubbles, 24 B per segment and 16 B per bubble
		// more resident, which a run that just fits the device does not have.
		const int STAGES_LINKS_FIRST[GraphFormat::TABLES] = {GraphFormat::COLORS, GraphFormat::LINKS, GraphFormat::BUBBLES, GraphFormat::DISTANCES, GraphFormat::COMPONENTS,
			GraphFormat::SUPERBUBBLES, GraphFormat::ANCHORS, GraphFormat::LOCATE, GraphFormat::CLASSES, GraphFormat::TRACKS, GraphFormat::VARIANTS};
		const int STAGES_DISTANCES_FIRST[GraphFormat::TABLES] = {GraphFormat::COLORS, GraphFormat::DISTANCES, GraphFormat::LINKS, GraphFormat::BUBBLES, GraphFormat::COMPONENTS,
			GraphFormat::SUPERBUBBLES, GraphFormat::ANCHORS, GraphFormat::LOCATE, GraphFormat::CLASSES, GraphFormat::TRACKS, GraphFormat::VARIANTS};

		// The caller's clock and [timing] lines.  built: after a stage's build, with the stage and its TPC_K_* (EDGES, then LOCATE
		// once its batches are through: their kernel time is locateKernelMs, not the last batch's); fetched: after a stage's fetch.
		struct StageObserver
		{
			std::function<void(int stage, int kernel)> built;
			std::function<void(int stage)> fetched;
			uint64_t locateBatches;
			double locateKernelMs;
			StageObserver() : locateBatches(0), locateKernelMs(0) {}
		};

		// "<the><noun> stage and the <other> disagree about the <what>": `the` opens the sentence, and the distance stage's other
		// party is called the caller's way
		struct StageWording
		{
			const char * the;
			const char * colorsOfDistances;
		};

		// The wanted stages over the segment table on the device, in `order`, each fetched as far as the files print it
		// (tablerequest.h: NeedsColorRows, NeedsLinkRows).  counts: tpc_segments_counts; t.map and the queries are the caller's
		// (MakeColorMap, LoadQueries); linkBits: the link stage runs in any case and its first bits are fetched (the compact text).
		inline void BuildTables(const Api & api, const GraphFormat::TableRequest & request, const int * order, const uint64_t * counts, bool linkBits, uint64_t batchPositions,
			const StageWording & wording, GraphFormat::Tables & t, StageObserver & observer)
		{
			using namespace GraphFormat;
			auto agree = [&wording](bool same, const char * noun, const char * other, const char * what)
			{
				if (!same) throw std::runtime_error(std::string(wording.the) + noun + " stage and the " + other + " disagree about the " + what);
			};

			const uint64_t events = counts[0];
			t.segments = counts[1];
			for (int at = 0; at < TABLES; at++)
			{
				const int stage = order[at];
				if (stage == COLORS ? !NeedsColorBuild(request) : stage == LINKS ? !NeedsLinkBuild(request) && !linkBits : stage == SUPERBUBBLES ? !NeedsSuperbubbleBuild(request) : !request.On(TableId(stage))) continue;
				switch (stage)
				{
				case COLORS:
					BuildColors(api, t.map);
					observer.built(stage, TPC_K_COLORS);
					if (NeedsColorRows(request)) FetchColors(api, t.map, t.segments, t.colors);
					break;
				case LINKS:
					BuildLinks(api);
					observer.built(stage, TPC_K_LINKS);
					t.linkRows = FetchLinks(api, events, NeedsLinkRows(request), linkBits, t.links);
					break;
				case BUBBLES:
					BuildBubbles(api);
					observer.built(stage, TPC_K_BUBBLES);
					FetchBubbles(api, t.bubbles);
					break;
				case DISTANCES:
					BuildDistances(api);
					observer.built(stage, TPC_K_DISTANCES);
					agree(FetchDistances(api, t.map.label.size(), t.segments, t.distances), "distance", wording.colorsOfDistances, "colours or the segments");
					break;
				case COMPONENTS:
					BuildComponents(api);
					observer.built(stage, TPC_K_COMPONENTS);
					agree(FetchComponents(api, t.segments, t.colors.Words(), t.components), "component", "segment table", "segments");
					break;
				case SUPERBUBBLES:
					BuildSuperbubbles(api, request.superbubblesMax);
					observer.built(stage, TPC_K_SUPERBUBBLES);
					agree(FetchSuperbubbles(api, t.segments, t.colors.Words(), t.superbubbles), "superbubble", "segment table", "segments");
					break;
				case ANCHORS:
					BuildAnchors(api, t.map, request.anchorsRef);
					observer.built(stage, TPC_K_ANCHORS);
					agree(FetchAnchors(api, t.map, events, t.segments, t.anchors), "anchor", "colour map", "colours");
					break;
				case CLASSES:
					BuildClasses(api);
					observer.built(stage, TPC_K_CLASSES);
					agree(FetchClasses(api, t.segments, t.colors.Words(), t.classes), "class", "segment table", "segments");
					break;
				case TRACKS:
					BuildTracks(api, t.map, request.tracksOf);
					observer.built(stage, TPC_K_TRACKS);
					agree(FetchTracks(api, t.map, t.segments, t.tracks), "track", "colour map", "colours");
					break;
				case VARIANTS:
					BuildVariants(api, t.map, request.variantsRef);
					observer.built(stage, TPC_K_VARIANTS);
					agree(FetchVariants(api, t.map, t.segments, t.superbubbles.Rows(), t.variants), "variant", "colour map", "colours or the superbubbles");
					break;
				case LOCATE:
					uint64_t edges[6] = {0, 0, 0, 0, 0, 0};
					BuildEdges(api, edges);
					observer.built(EDGES, TPC_K_LOCATE);
					observer.locateBatches = LocateOnDevice(api, edges, t.map.label.size(), t.segments, t.queryLetters, batchPositions, t.locate, observer.locateKernelMs);
					observer.built(stage, TPC_K_LOCATE);
					break;
				}

				observer.fetched(stage);
			}
		}
	}
}

#endif
