// graphformat.cpp -- see graphformat.h.
#include "graphformat.h"

#include <algorithm>
#include <cerrno>
#include <condition_variable>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <unordered_map>

#include <fcntl.h>
#include <unistd.h>

#include "streamfastaparser.h"

namespace TwoPaCo
{
	namespace GraphFormat
	{
		void LoadSequences(const std::vector<std::string> & fasta, bool prefixed, size_t threads, InputSequences & seq, LoadedSequences & loaded)
		{
			struct PerFile
			{
				std::vector<std::string> name, body;
				std::vector<std::vector<uint64_t> > ambiguous;
				std::string error;
			};

			std::vector<PerFile> file(fasta.size());
			RunParallel(fasta.size(), threads, [&](size_t f)
			{
				PerFile & out = file[f];
				try
				{
					TwoPaCo::StreamFastaParser parser(fasta[f]);
					while (parser.ReadRecord())
					{
						// "s0_": the reference never advances its file counter, every prefix is "s0_" (graphdump.cpp:176-192)
						out.name.push_back(prefixed ? "s0_" + parser.GetCurrentHeader() : parser.GetCurrentHeader());
						std::string body;
						std::vector<uint64_t> ambiguous;
						for (char ch; parser.GetChar(ch);)
						{
							if (!DnaChar::IsDefinite(ch) && ch != 'N') ambiguous.push_back(body.size());
							body.push_back(ch);
						}

						out.body.push_back(std::string());
						out.body.back().swap(body);
						out.ambiguous.push_back(std::vector<uint64_t>());
						out.ambiguous.back().swap(ambiguous);
					}
				}
				catch (std::runtime_error & e)
				{
					out.error = e.what();
					if (out.error.empty()) out.error = "unreadable FASTA file";
				}
			});

			for (size_t f = 0; f < fasta.size(); f++)
			{
				// the serial walk meets the records of a broken file before its error; what it reports is the first error in file order
				if (!file[f].error.empty()) throw std::runtime_error(file[f].error);
				for (size_t r = 0; r < file[f].name.size(); r++)
				{
					seq.name.push_back(file[f].name[r]);
					seq.file[file[f].name[r]] = fasta[f];
					seq.fileIndex.push_back(uint32_t(f));
					seq.length.push_back(file[f].body[r].size());
					loaded.body.push_back(std::string());
					loaded.body.back().swap(file[f].body[r]);
					loaded.ambiguous.push_back(std::vector<uint64_t>());
					loaded.ambiguous.back().swap(file[f].ambiguous[r]);
				}
			}
		}

		bool IsGraphFormat(const std::string & format)
		{
			return format == "gfa1" || format == "gfa2" || format == "fasta";
		}

		void HeaderLines(const std::string & format, const InputSequences & seq, Out & out, bool compact)
		{
			if (format == "gfa1")
			{
				out << "H\tVN:Z:1.0\n";
				if (!compact) for (const std::string & name : seq.name) out << "S\t" << name << "\t*\tUR:Z:" << seq.file.find(name)->second << '\n';
			}

			if (format == "gfa2") out << "H\tVN:Z:2.0\n";
		}

		namespace
		{
			// about eight chunks per thread, of 16 .. 65536 events (a few MB of text at most): small inputs are cut as well
			uint64_t ChunkEvents(uint64_t events, size_t threads)
			{
				return std::max<uint64_t>(16, std::min<uint64_t>(uint64_t(1) << 16, events / (8 * threads) + 1));
			}

			SegmentSink * MakeSink(const std::string & format, Out & out, const InputSequences & seq, GfaSink * & gfa, CompactGfa1Sink * & compact, bool wantCompact)
			{
				gfa = 0;
				compact = 0;
				if (format == "gfa1" && wantCompact) return gfa = compact = new CompactGfa1Sink(out, seq);
				if (format == "gfa1") return gfa = new Gfa1Sink(out, seq);
				if (format == "gfa2") return gfa = new Gfa2Sink(out, seq);
				return new FastaSink(out);
			}

			// the sequence that holds event e: the last s with seqEventBegin[s] <= e (sequences without events share their entry
			// with the next one that has some)
			size_t SequenceOf(const EventTable & t, uint64_t e)
			{
				const uint32_t * b = t.seqEventBegin;
				return size_t(std::upper_bound(b, b + t.sequences + 1, e, [](uint64_t v, uint32_t x) { return v < uint64_t(x); }) - b) - 1;
			}

			void FormatChunk(const EventTable & t, const InputSequences & seq, const LoadedSequences & loaded, size_t k, const std::string & format,
				uint64_t e0, uint64_t e1, std::string & into)
			{
				Out chunkOut(false);
				GfaSink * gfa = 0;
				CompactGfa1Sink * compact = 0;
				std::unique_ptr<SegmentSink> sink(MakeSink(format, chunkOut, seq, gfa, compact, t.linkFirst != 0));
				size_t sequence = e0 < e1 ? SequenceOf(t, e0) : 0;
				for (uint64_t e = e0; e < e1; e++)
				{
					while (e >= t.seqEventBegin[sequence + 1]) ++sequence;
					SegmentEvent ev;
					ev.id = t.name[e];
					ev.begin = t.begin[e];
					ev.end = t.end[e];
					ev.size = ev.end + k - ev.begin;
					ev.first = (t.first[e >> 5] >> (e & 31)) & 1u;
					ev.sequence = sequence;
					if (e == e0 && gfa)
					{
						// the event before lies in the same sequence: the link to it is this chunk's
						if (e > t.seqEventBegin[sequence]) gfa->Resume(t.name[e - 1], uint64_t(t.end[e - 1]) + k - t.begin[e - 1]);
						else gfa->Resume(0, 0);
					}

					if (compact) compact->NextLink((t.linkFirst[e >> 5] >> (e & 31)) & 1u);
					sink->Segment(ev, loaded.body[sequence], k);
					if (gfa && e + 1 == t.seqEventBegin[sequence + 1])
					{
						// last event of its sequence: the path line is this worker's, whatever chunk the path began in
						const uint64_t begin = t.seqEventBegin[sequence];
						gfa->EndOfSequence(sequence, t.name + begin, size_t(e - begin + 1));
					}
				}

				into.swap(chunkOut.Text());
			}

			bool WriteAll(int fd, const char * data, size_t n, uint64_t offset)
			{
				for (size_t done = 0; done < n;)
				{
					const ssize_t w = ::pwrite(fd, data + done, n - done, off_t(offset + done));
					if (w < 0 && errno == EINTR) continue;
					if (w <= 0) return false;
					done += size_t(w);
				}

				return true;
			}
		}

		void CheckEventTable(const EventTable & t, const LoadedSequences & loaded, size_t k, size_t threads)
		{
			if (t.events >= UINT32_MAX) throw std::runtime_error("event table: event indices are 32 bits");
			if (t.events && (!t.name || !t.first || !t.begin || !t.end)) throw std::runtime_error("event table: arrays required");
			if (!t.seqEventBegin) throw std::runtime_error("event table: sequence ranges required");
			if (t.sequences != loaded.body.size())
			{
				throw std::runtime_error("event table: made for " + std::to_string(t.sequences) + " sequences, the FASTA files hold " + std::to_string(loaded.body.size()));
			}

			if (t.seqEventBegin[0] != 0 || t.seqEventBegin[t.sequences] != t.events) throw std::runtime_error("event table: the sequences' event ranges do not cover the events");
			for (uint64_t s = 0; s < t.sequences; s++)
			{
				if (t.seqEventBegin[s] > t.seqEventBegin[s + 1]) throw std::runtime_error("event table: the sequences' event ranges must ascend");
			}

			const size_t parts = std::max<size_t>(1, std::min<size_t>(threads, size_t(t.events / 65536 + 1)));
			std::vector<uint64_t> bad(parts, UINT64_MAX);
			RunParallel(parts, parts, [&](size_t p)
			{
				const uint64_t e0 = t.events * p / parts, e1 = t.events * (p + 1) / parts;
				size_t sequence = e0 < e1 ? SequenceOf(t, e0) : 0;
				for (uint64_t e = e0; e < e1; e++)
				{
					while (e >= t.seqEventBegin[sequence + 1]) ++sequence;
					if (t.end[e] <= t.begin[e] || uint64_t(t.end[e]) + k > loaded.body[sequence].size())
					{
						bad[p] = e;
						break;
					}
				}
			});

			for (uint64_t e : bad)
			{
				if (e != UINT64_MAX) throw std::runtime_error("event table: event " + std::to_string(e) + " does not lie inside its sequence");
			}
		}

		uint64_t FormatEvents(const EventTable & t, const InputSequences & seq, const LoadedSequences & loaded, size_t k, const std::string & format,
			size_t threads, int fd, uint64_t fileOffset)
		{
			threads = std::max<size_t>(1, threads);
			const uint64_t events = t.events;
			const uint64_t chunkEvents = ChunkEvents(events, threads);
			const size_t chunks = size_t((events + chunkEvents - 1) / chunkEvents);
			auto formatChunk = [&](size_t c, std::string & into)
			{
				const uint64_t e0 = uint64_t(c) * chunkEvents;
				FormatChunk(t, seq, loaded, k, format, e0, std::min(events, e0 + chunkEvents), into);
			};

			uint64_t total = 0;
			if (threads <= 1 || chunks <= 1)
			{
				for (size_t c = 0; c < chunks; c++)
				{
					std::string textOfChunk;
					formatChunk(c, textOfChunk);
					if (fd < 0) std::fwrite(textOfChunk.data(), 1, textOfChunk.size(), stdout);
					else if (!WriteAll(fd, textOfChunk.data(), textOfChunk.size(), fileOffset + total)) throw std::runtime_error("Can't write to the graph file");
					total += textOfChunk.size();
				}
			}
			else if (fd >= 0)
			{
				// Every worker writes its own chunk.  Chunks are taken in order, so the sizes of the chunks before c are known as
				// soon as the workers holding them have formatted theirs: a worker waits only for chunks that are already running.
				// The space is preallocated in doubling steps ahead of the frontier (the size of the text is not known before
				// it is formatted); the caller truncates the file to what was written.
				std::vector<uint64_t> offset(chunks + 1, 0);
				std::mutex lock;
				std::condition_variable changed;
				size_t known = 0;            // offset[0 .. known] are final
				uint64_t allocated = 0;
				bool failed = false;
				std::atomic<size_t> cursor(0);
				auto work = [&]()
				{
					for (size_t c = cursor++; c < chunks; c = cursor++)
					{
						std::string textOfChunk;
						formatChunk(c, textOfChunk);
						uint64_t at = 0;
						{
							std::unique_lock<std::mutex> hold(lock);
							changed.wait(hold, [&]() { return known >= c; });
							at = offset[c];
							offset[c + 1] = at + textOfChunk.size();
							known = c + 1;
							if (offset[c + 1] > allocated)
							{
								const uint64_t upTo = std::max<uint64_t>(offset[c + 1] + (uint64_t(8) << 20), 2 * allocated);
								(void)::posix_fallocate(fd, off_t(fileOffset + allocated), off_t(upTo - allocated));  // a file system without it: the writes extend the file
								allocated = upTo;
							}
						}

						changed.notify_all();
						if (!WriteAll(fd, textOfChunk.data(), textOfChunk.size(), fileOffset + at))
						{
							std::unique_lock<std::mutex> hold(lock);
							failed = true;
						}
					}
				};

				std::vector<std::thread> pool;
				for (size_t w = 1; w < std::min(threads, chunks); w++) pool.emplace_back(work);
				work();
				for (std::thread & th : pool) th.join();
				if (failed) throw std::runtime_error("Can't write to the graph file");
				total = offset[chunks];
			}
			else
			{
				// threads - 1 workers format, this thread writes; a worker runs at most `window` chunks ahead of the writer
				std::vector<std::string> done(chunks);
				std::vector<char> ready(chunks, 0);
				std::mutex lock;
				std::condition_variable changed;
				size_t written = 0;
				const size_t window = 4 * threads;
				std::atomic<size_t> cursor(0);
				std::vector<std::thread> pool;
				for (size_t w = 1; w < threads; w++)
				{
					pool.emplace_back([&]()
					{
						for (size_t c = cursor++; c < chunks; c = cursor++)
						{
							{
								std::unique_lock<std::mutex> hold(lock);
								changed.wait(hold, [&]() { return c < written + window; });
							}

							std::string textOfChunk;
							formatChunk(c, textOfChunk);
							{
								std::unique_lock<std::mutex> hold(lock);
								done[c].swap(textOfChunk);
								ready[c] = 1;
							}

							changed.notify_all();
						}
					});
				}

				for (size_t c = 0; c < chunks; c++)
				{
					std::string textOfChunk;
					{
						std::unique_lock<std::mutex> hold(lock);
						changed.wait(hold, [&]() { return ready[c] != 0; });
						textOfChunk.swap(done[c]);
					}

					std::fwrite(textOfChunk.data(), 1, textOfChunk.size(), stdout);
					total += textOfChunk.size();
					{
						std::unique_lock<std::mutex> hold(lock);
						written = c + 1;
					}

					changed.notify_all();
				}

				for (std::thread & th : pool) th.join();
			}

			if (fd < 0) std::fflush(stdout);
			return total;
		}

		void WriteGraphFileWith(const std::string & format, const InputSequences & seq, const std::string & outPath,
			const std::function<uint64_t(int fd, uint64_t fileOffset)> & events, bool compact)
		{
			int fd = ::open(outPath.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
			if (fd < 0) throw std::runtime_error("Can't create the graph file " + outPath);
			try
			{
				Out head(false);
				HeaderLines(format, seq, head, compact);
				if (!WriteAll(fd, head.Text().data(), head.Text().size(), 0)) throw std::runtime_error("Can't write to the graph file");
				const uint64_t size = head.Text().size() + events(fd, head.Text().size());
				if (::ftruncate(fd, off_t(size)) != 0) throw std::runtime_error("Can't write to the graph file");
				const int closing = fd;
				fd = -1;
				if (::close(closing) != 0) throw std::runtime_error("Can't write to the graph file");
			}
			catch (...)
			{
				if (fd >= 0) ::close(fd);
				::unlink(outPath.c_str());
				throw;
			}
		}

		void MakeColorMap(const InputSequences & seq, const std::vector<std::string> & fasta, bool bySequence, ColorMap & out)
		{
			if (seq.fileIndex.size() != seq.name.size()) throw std::runtime_error("colour table: the file of every sequence is required");
			out.bySequence = bySequence;
			out.colorOfSequence.clear();
			out.label.clear();
			for (size_t s = 0; s < seq.name.size(); s++)
			{
				out.colorOfSequence.push_back(bySequence ? uint32_t(s) : seq.fileIndex[s]);
				if (bySequence) out.label.push_back(std::to_string(s + 1) + "\t" + fasta[seq.fileIndex[s]]);
			}

			if (!bySequence) out.label = fasta;
		}

		void ComputeColors(const EventTable & t, size_t k, const std::vector<uint32_t> & colorOfSequence, uint64_t colors, ColorTable & out)
		{
			if (colors == 0) throw std::runtime_error("colour table: at least one colour is required");
			if (colorOfSequence.size() != t.sequences) throw std::runtime_error("colour table: the colour of every sequence is required");
			for (uint32_t c : colorOfSequence)
			{
				if (c >= colors) throw std::runtime_error("colour table: a sequence has the colour " + std::to_string(c) + ", there are " + std::to_string(colors) + " colours");
			}

			if (!t.seqEventBegin || t.seqEventBegin[0] != 0 || t.seqEventBegin[t.sequences] != t.events) throw std::runtime_error("event table: the sequences' event ranges do not cover the events");
			out = ColorTable();
			out.colors = colors;
			const size_t words = out.Words();
			const int64_t FRESH = int64_t(1) << 34;
			std::unordered_map<int64_t, uint32_t> rowOf;
			size_t sequence = 0;
			for (uint64_t e = 0; e < t.events; e++)
			{
				while (e >= t.seqEventBegin[sequence + 1]) ++sequence;
				const int64_t name = Magnitude(t.name[e]);
				uint32_t row = 0;
				std::unordered_map<int64_t, uint32_t>::const_iterator seen = name >= FRESH ? rowOf.end() : rowOf.find(name);
				if (seen == rowOf.end())
				{
					row = uint32_t(out.firstEvent.size());
					if (name < FRESH) rowOf[name] = row;
					out.firstEvent.push_back(uint32_t(e));
					out.occurrences.push_back(0);
					out.forward.push_back(0);
					out.presence.resize(out.presence.size() + words, 0);
				}
				else row = seen->second;

				const uint32_t c = colorOfSequence[sequence];
				out.occurrences[row] += 1;
				if (t.name[e] > 0) out.forward[row] += 1;
				out.presence[size_t(row) * words + (c >> 5)] |= uint32_t(1) << (c & 31);
			}

			out.histSegments.assign(colors + 1, 0);
			out.histBases.assign(colors + 1, 0);
			for (size_t r = 0; r < out.Rows(); r++)
			{
				uint32_t n = 0;
				for (size_t w = 0; w < words; w++) n += uint32_t(__builtin_popcount(out.presence[r * words + w]));
				out.nColors.push_back(n);
				const uint32_t e0 = out.firstEvent[r];
				out.histSegments[n] += 1;
				out.histBases[n] += uint64_t(t.end[e0]) - t.begin[e0] + k;
			}
		}

		void WriteColors(const EventTable & t, size_t k, const ColorMap & map, const ColorTable & colors, const std::string & path)
		{
			const size_t rows = colors.Rows(), words = colors.Words();
			if (colors.occurrences.size() != rows || colors.forward.size() != rows || colors.nColors.size() != rows || colors.presence.size() != rows * words ||
				colors.histSegments.size() != colors.colors + 1 || colors.histBases.size() != colors.colors + 1 || map.label.size() != colors.colors)
			{
				throw std::runtime_error("colour table: the arrays do not agree about the rows and the colours");
			}

			for (uint32_t e0 : colors.firstEvent)
			{
				if (e0 >= t.events) throw std::runtime_error("colour table: a row's first event lies outside the event table");
			}

			std::FILE * f = path.empty() ? stdout : std::fopen(path.c_str(), "wb");
			if (!f) throw std::runtime_error("Can't create the colour table " + path);
			std::string buf;
			bool good = true;
			auto flush = [&]() { good = good && std::fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); };
			buf += "#twopaco-colors\t1\tby=" + std::string(map.bySequence ? "sequence" : "file") + "\tk=" + std::to_string(k) + "\tcolors=" + std::to_string(colors.colors) +
				"\tsegments=" + std::to_string(rows) + "\tevents=" + std::to_string(t.events) + "\n";
			for (uint64_t c = 0; c < colors.colors; c++) buf += "#color\t" + std::to_string(c) + "\t" + map.label[c] + "\n";
			const size_t digits = size_t((colors.colors + 3) / 4);
			for (size_t r = 0; r < rows; r++)
			{
				const uint32_t e0 = colors.firstEvent[r];
				buf += std::to_string(static_cast<long long>(Magnitude(t.name[e0])));
				buf += '\t';
				buf += std::to_string(static_cast<unsigned long long>(uint64_t(t.end[e0]) - t.begin[e0] + k));
				buf += '\t';
				buf += std::to_string(colors.occurrences[r]);
				buf += '\t';
				buf += std::to_string(colors.forward[r]);
				buf += '\t';
				buf += std::to_string(colors.nColors[r]);
				buf += '\t';
				const uint32_t * p = &colors.presence[r * words];
				for (size_t j = 0; j < digits; j++) buf += "0123456789abcdef"[(p[j >> 3] >> (4 * (j & 7))) & 15u];
				buf += '\n';
				if (buf.size() > (size_t(1) << 20)) flush();
			}

			for (uint64_t n = 1; n <= colors.colors; n++)
			{
				if (colors.histSegments[n]) buf += "#hist\t" + std::to_string(n) + "\t" + std::to_string(colors.histSegments[n]) + "\t" + std::to_string(colors.histBases[n]) + "\n";
			}

			flush();
			good = good && std::fflush(f) == 0;
			if (f != stdout) good = (std::fclose(f) == 0) && good;
			if (!good)
			{
				if (f != stdout) ::unlink(path.c_str());
				throw std::runtime_error("Can't write the colour table");
			}
		}

		namespace
		{
			struct LinkClass
			{
				int64_t from, to;
				bool operator == (const LinkClass & o) const { return from == o.from && to == o.to; }
			};

			struct LinkClassHash
			{
				size_t operator () (const LinkClass & c) const
				{
					uint64_t x = uint64_t(c.from) * 0x9e3779b97f4a7c15ull ^ (uint64_t(c.to) + 0x7f4a7c15ull);
					x ^= x >> 31; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 29;
					return size_t(x);
				}
			};
		}

		void ComputeLinks(const EventTable & t, LinkTable & out)
		{
			if (!t.seqEventBegin || t.seqEventBegin[0] != 0 || t.seqEventBegin[t.sequences] != t.events) throw std::runtime_error("event table: the sequences' event ranges do not cover the events");
			out = LinkTable();
			out.linkFirst.assign(size_t((t.events + 31) / 32), 0);
			std::unordered_map<LinkClass, uint32_t, LinkClassHash> rowOf;
			size_t sequence = 0;
			for (uint64_t e = 0; e < t.events; e++)
			{
				while (e >= t.seqEventBegin[sequence + 1]) ++sequence;
				if (e == t.seqEventBegin[sequence]) continue;   // the first event of its sequence closes no link
				const LinkClass spelled = {t.name[e - 1], t.name[e]}, reversed = {-t.name[e], -t.name[e - 1]};
				const bool keep = spelled.from < reversed.from || (spelled.from == reversed.from && spelled.to <= reversed.to);
				const LinkClass key = keep ? spelled : reversed;
				out.occurrences += 1;
				std::unordered_map<LinkClass, uint32_t, LinkClassHash>::const_iterator seen = rowOf.find(key);
				uint32_t row = 0;
				if (seen == rowOf.end())
				{
					row = uint32_t(out.firstEvent.size());
					rowOf[key] = row;
					out.firstEvent.push_back(uint32_t(e));
					out.count.push_back(0);
					out.same.push_back(0);
					out.linkFirst[e >> 5] |= uint32_t(1) << (e & 31);
				}
				else row = seen->second;

				const uint32_t e0 = out.firstEvent[row];
				out.count[row] += 1;
				if (t.name[e0 - 1] == spelled.from && t.name[e0] == spelled.to) out.same[row] += 1;
			}
		}

		void WriteLinks(const EventTable & t, size_t k, uint64_t segments, const LinkTable & links, const std::string & path)
		{
			const size_t rows = links.Rows();
			if (links.count.size() != rows || links.same.size() != rows) throw std::runtime_error("link table: the arrays do not agree about the rows");
			for (uint32_t e0 : links.firstEvent)
			{
				if (e0 == 0 || e0 >= t.events) throw std::runtime_error("link table: a row's first event lies outside the event table");
			}

			std::FILE * f = path.empty() ? stdout : std::fopen(path.c_str(), "wb");
			if (!f) throw std::runtime_error("Can't create the link table " + path);
			std::string buf;
			bool good = true;
			auto flush = [&]() { good = good && std::fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); };
			buf += "#twopaco-links\t1\tk=" + std::to_string(k) + "\tsegments=" + std::to_string(segments) + "\tlinks=" + std::to_string(rows) + "\toccurrences=" +
				std::to_string(links.occurrences) + "\n";
			for (size_t r = 0; r < rows; r++)
			{
				const uint32_t e0 = links.firstEvent[r];
				const int64_t from = t.name[e0 - 1], to = t.name[e0];
				buf += std::to_string(static_cast<long long>(Magnitude(from)));
				buf += '\t';
				buf += Strand(from);
				buf += '\t';
				buf += std::to_string(static_cast<long long>(Magnitude(to)));
				buf += '\t';
				buf += Strand(to);
				buf += '\t';
				buf += std::to_string(links.count[r]);
				buf += '\t';
				buf += std::to_string(links.same[r]);
				buf += '\n';
				if (buf.size() > (size_t(1) << 20)) flush();
			}

			flush();
			good = good && std::fflush(f) == 0;
			if (f != stdout) good = (std::fclose(f) == 0) && good;
			if (!good)
			{
				if (f != stdout) ::unlink(path.c_str());
				throw std::runtime_error("Can't write the link table");
			}
		}

		void ComputeBubbles(const EventTable & t, const LinkTable & links, BubbleTable & out)
		{
			out = BubbleTable();
			// the row of every segment: the order of the first sights, as ComputeColors numbers them
			const int64_t FRESH = int64_t(1) << 34;
			std::unordered_map<int64_t, uint32_t> rowOf;
			std::vector<uint32_t> rowOfEvent(size_t(t.events), 0);
			uint64_t rows = 0;
			for (uint64_t e = 0; e < t.events; e++)
			{
				const int64_t name = Magnitude(t.name[e]);
				std::unordered_map<int64_t, uint32_t>::const_iterator seen = name >= FRESH ? rowOf.end() : rowOf.find(name);
				if (seen == rowOf.end())
				{
					if (name < FRESH) rowOf[name] = uint32_t(rows);
					rowOfEvent[e] = uint32_t(rows++);
				}
				else rowOfEvent[e] = seen->second;
			}

			if (rows > (uint64_t(1) << 31)) throw std::runtime_error("bubble table: " + std::to_string(rows) + " segments, a side holds at most 2147483648");
			out.sides = 2 * rows;
			auto side = [&](uint64_t e) { return uint32_t(rowOfEvent[e] << 1 | (t.name[e] < 0 ? 1u : 0u)); };
			auto rev = [](uint32_t code) { return code ^ 1u; };
			std::vector<std::set<uint32_t> > outSet(size_t(out.sides));
			for (uint32_t e0 : links.firstEvent)
			{
				if (e0 == 0 || e0 >= t.events) throw std::runtime_error("link table: a row's first event lies outside the event table");
				const uint32_t from = side(e0 - 1), to = side(e0);
				outSet[from].insert(to);
				outSet[rev(to)].insert(rev(from));   // the same arc once more when the link is its own reverse: a set holds it once
			}

			for (const std::set<uint32_t> & heads : outSet)
			{
				out.arcs += heads.size();
				out.hist[std::min<size_t>(heads.size(), 5)] += 1;
			}

			auto deg = [&](uint32_t u) { return outSet[u].size(); };
			for (uint64_t code = 0; code < out.sides; code++)
			{
				const uint32_t s = uint32_t(code);
				if (deg(s) != 2) continue;
				const uint32_t a = *outSet[s].begin(), b = *outSet[s].rbegin();   // a < b: the arm order
				if (deg(rev(a)) != 1 || deg(rev(b)) != 1) continue;
				if (deg(a) != 1 || deg(b) != 1 || outSet[a] != outSet[b]) continue;
				const uint32_t sink = *outSet[a].begin();
				if (deg(rev(sink)) != 2) continue;
				const std::set<uint32_t> four = {s >> 1, a >> 1, b >> 1, sink >> 1};
				if (four.size() != 4) continue;
				if (!(s < rev(sink))) continue;   // found at rev(sink) as well: reported where the source code is the smaller
				out.source.push_back(s);
				out.armA.push_back(a);
				out.armB.push_back(b);
				out.sink.push_back(sink);
			}
		}

		void WriteBubbles(const EventTable & t, size_t k, const ColorMap & map, const ColorTable & colors, uint64_t links, const BubbleTable & bubbles,
			const std::string & path)
		{
			const size_t rows = colors.Rows(), words = colors.Words(), n = bubbles.Rows();
			if (colors.occurrences.size() != rows || colors.nColors.size() != rows || colors.presence.size() != rows * words || map.label.size() != colors.colors)
			{
				throw std::runtime_error("colour table: the arrays do not agree about the rows and the colours");
			}

			if (bubbles.armA.size() != n || bubbles.armB.size() != n || bubbles.sink.size() != n) throw std::runtime_error("bubble table: the arrays do not agree about the rows");
			if (bubbles.sides != 2 * uint64_t(rows)) throw std::runtime_error("bubble table: its sides are not those of the colour table's rows");
			for (uint32_t e0 : colors.firstEvent)
			{
				if (e0 >= t.events) throw std::runtime_error("colour table: a row's first event lies outside the event table");
			}

			for (const std::vector<uint32_t> * codes : {&bubbles.source, &bubbles.armA, &bubbles.armB, &bubbles.sink})
			{
				for (uint32_t code : *codes)
				{
					if (code >= bubbles.sides) throw std::runtime_error("bubble table: a side lies outside the segments");
				}
			}

			std::FILE * f = path.empty() ? stdout : std::fopen(path.c_str(), "wb");
			if (!f) throw std::runtime_error("Can't create the bubble table " + path);
			std::string buf;
			bool good = true;
			auto flush = [&]() { good = good && std::fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); };
			buf += "#twopaco-bubbles\t1\tby=" + std::string(map.bySequence ? "sequence" : "file") + "\tk=" + std::to_string(k) + "\tcolors=" + std::to_string(colors.colors) +
				"\tsegments=" + std::to_string(rows) + "\tlinks=" + std::to_string(links) + "\tbubbles=" + std::to_string(n) + "\n";
			for (uint64_t c = 0; c < colors.colors; c++) buf += "#color\t" + std::to_string(c) + "\t" + map.label[c] + "\n";
			for (size_t d = 0; d < 6; d++)
			{
				if (bubbles.hist[d]) buf += "#sides\t" + std::to_string(d) + (d == 5 ? "+" : "") + "\t" + std::to_string(bubbles.hist[d]) + "\n";
			}

			const size_t digits = size_t((colors.colors + 3) / 4);
			auto side = [&](uint32_t code)
			{
				buf += std::to_string(static_cast<long long>(Magnitude(t.name[colors.firstEvent[code >> 1]])));
				buf += '\t';
				buf += (code & 1u) ? '-' : '+';
				buf += '\t';
			};

			auto hex = [&](uint32_t row)
			{
				const uint32_t * p = &colors.presence[size_t(row) * words];
				for (size_t j = 0; j < digits; j++) buf += "0123456789abcdef"[(p[j >> 3] >> (4 * (j & 7))) & 15u];
			};

			for (size_t r = 0; r < n; r++)
			{
				const uint32_t a = bubbles.armA[r] >> 1, b = bubbles.armB[r] >> 1;
				side(bubbles.source[r]);
				side(bubbles.armA[r]);
				side(bubbles.armB[r]);
				side(bubbles.sink[r]);
				const uint32_t ea = colors.firstEvent[a], eb = colors.firstEvent[b];
				buf += std::to_string(static_cast<unsigned long long>(uint64_t(t.end[ea]) - t.begin[ea] + k));
				buf += '\t';
				buf += std::to_string(static_cast<unsigned long long>(uint64_t(t.end[eb]) - t.begin[eb] + k));
				buf += '\t';
				buf += std::to_string(colors.occurrences[a]);
				buf += '\t';
				buf += std::to_string(colors.occurrences[b]);
				buf += '\t';
				buf += std::to_string(colors.nColors[a]);
				buf += '\t';
				buf += std::to_string(colors.nColors[b]);
				buf += '\t';
				hex(a);
				buf += '\t';
				hex(b);
				buf += '\t';
				uint32_t both = 0;
				for (size_t w = 0; w < words; w++) both += uint32_t(__builtin_popcount(colors.presence[size_t(a) * words + w] & colors.presence[size_t(b) * words + w]));
				buf += std::to_string(both);
				buf += '\n';
				if (buf.size() > (size_t(1) << 20)) flush();
			}

			flush();
			good = good && std::fflush(f) == 0;
			if (f != stdout) good = (std::fclose(f) == 0) && good;
			if (!good)
			{
				if (f != stdout) ::unlink(path.c_str());
				throw std::runtime_error("Can't write the bubble table");
			}
		}

		void ComputeDistances(const EventTable & t, const ColorTable & colors, DistanceTable & out)
		{
			const size_t rows = colors.Rows(), words = colors.Words(), n = size_t(colors.colors);
			if (colors.presence.size() != rows * words) throw std::runtime_error("colour table: the arrays do not agree about the rows and the colours");
			out = DistanceTable();
			out.colors = colors.colors;
			out.segments.assign(n * n, 0);
			out.edges.assign(n * n, 0);
			std::vector<uint32_t> held;
			for (size_t r = 0; r < rows; r++)
			{
				const uint32_t e0 = colors.firstEvent[r];
				if (e0 >= t.events) throw std::runtime_error("colour table: a row's first event lies outside the event table");
				const uint64_t weight = uint64_t(t.end[e0]) - t.begin[e0];
				held.clear();
				for (size_t c = 0; c < n; c++)
				{
					if ((colors.presence[r * words + (c >> 5)] >> (c & 31)) & 1u) held.push_back(uint32_t(c));
				}

				for (uint32_t i : held)
				{
					for (uint32_t j : held)
					{
						out.segments[size_t(i) * n + j] += 1;
						out.edges[size_t(i) * n + j] += weight;
					}
				}
			}
		}

		namespace
		{
			void CheckDistances(const ColorMap & map, const DistanceTable & d)
			{
				const size_t n = size_t(d.colors);
				if (d.segments.size() != n * n || d.edges.size() != n * n || map.label.size() != n) throw std::runtime_error("distance table: the arrays do not agree about the colours");
			}

			void WriteWhole(const std::string & buf, const std::string & path, const char * what)
			{
				std::FILE * f = path.empty() ? stdout : std::fopen(path.c_str(), "wb");
				if (!f) throw std::runtime_error(std::string("Can't create the ") + what + " " + path);
				bool good = std::fwrite(buf.data(), 1, buf.size(), f) == buf.size();
				good = good && std::fflush(f) == 0;
				if (f != stdout) good = (std::fclose(f) == 0) && good;
				if (!good)
				{
					if (f != stdout) ::unlink(path.c_str());
					throw std::runtime_error(std::string("Can't write the ") + what);
				}
			}
		}

		void WriteDistances(size_t k, const ColorMap & map, uint64_t rows, const DistanceTable & d, const std::string & path)
		{
			CheckDistances(map, d);
			const size_t n = size_t(d.colors);
			std::string buf;
			buf += "#twopaco-distances\t1\tby=" + std::string(map.bySequence ? "sequence" : "file") + "\tk=" + std::to_string(k) + "\tcolors=" + std::to_string(d.colors) +
				"\tsegments=" + std::to_string(rows) + "\n";
			for (size_t c = 0; c < n; c++) buf += "#color\t" + std::to_string(c) + "\t" + map.label[c] + "\n";
			for (size_t c = 0; c < n; c++) buf += "#self\t" + std::to_string(c) + "\t" + std::to_string(d.segments[c * n + c]) + "\t" + std::to_string(d.edges[c * n + c]) + "\n";
			for (size_t i = 0; i < n; i++)
			{
				for (size_t j = i + 1; j < n; j++)
				{
					buf += std::to_string(i);
					buf += '\t';
					buf += std::to_string(j);
					buf += '\t';
					buf += std::to_string(d.segments[i * n + j]);
					buf += '\t';
					buf += std::to_string(d.edges[i * n + j]);
					buf += '\n';
				}
			}

			WriteWhole(buf, path, "distance table");
		}

		void WriteDistancesPhylip(const ColorMap & map, const DistanceTable & d, const std::string & path)
		{
			CheckDistances(map, d);
			if (path.empty()) throw std::runtime_error("The PHYLIP matrix needs a file name");
			const size_t n = size_t(d.colors);
			std::string buf = std::to_string(n) + "\n";
			char number[64];
			for (size_t i = 0; i < n; i++)
			{
				for (char ch : map.label[i]) buf += static_cast<unsigned char>(ch) <= ' ' ? '_' : ch;
				for (size_t j = 0; j < n; j++)
				{
					const uint64_t shared = d.edges[i * n + j], u = d.edges[i * n + i] + d.edges[j * n + j] - shared;
					const double value = (i == j || u == 0) ? 0.0 : double(u - shared) / double(u);
					std::snprintf(number, sizeof number, " %.6f", value);
					buf += number;
				}

				buf += '\n';
			}

			WriteWhole(buf, path, "PHYLIP matrix");
		}

		void WriteDistanceFiles(size_t k, const ColorMap & map, uint64_t rows, const DistanceTable & d, const std::string & path, const std::string & phylipPath)
		{
			if (!phylipPath.empty()) WriteDistancesPhylip(map, d, phylipPath);
			try
			{
				WriteDistances(k, map, rows, d, path);
			}
			catch (...)
			{
				if (!phylipPath.empty()) ::unlink(phylipPath.c_str());
				throw;
			}
		}

		void ComputeComponents(const EventTable & t, size_t k, const LinkTable & links, const ColorTable & colors, ComponentTable & out)
		{
			out = ComponentTable();
			const size_t rows = colors.Rows(), words = colors.Words();
			if (colors.occurrences.size() != rows || colors.presence.size() != rows * words) throw std::runtime_error("colour table: the arrays do not agree about the rows and the colours");
			// the row of every segment: the order of the first sights, as ComputeColors numbers them
			const int64_t FRESH = int64_t(1) << 34;
			std::unordered_map<int64_t, uint32_t> rowOf;
			std::vector<uint32_t> rowOfEvent(size_t(t.events), 0);
			uint64_t seen = 0;
			for (uint64_t e = 0; e < t.events; e++)
			{
				const int64_t name = Magnitude(t.name[e]);
				std::unordered_map<int64_t, uint32_t>::const_iterator at = name >= FRESH ? rowOf.end() : rowOf.find(name);
				if (at == rowOf.end())
				{
					if (name < FRESH) rowOf[name] = uint32_t(seen);
					rowOfEvent[e] = uint32_t(seen++);
				}
				else rowOfEvent[e] = at->second;
			}

			if (seen != rows) throw std::runtime_error("component table: the colour table's rows are not the segments of the event table");
			if (rows >= (uint64_t(1) << 31)) throw std::runtime_error("component table: " + std::to_string(rows) + " segments, a row holds at most 2147483647");
			// union-find: the smaller root stays the root, so a tree's root is its smallest row
			std::vector<uint32_t> parent(rows);
			for (size_t r = 0; r < rows; r++) parent[r] = uint32_t(r);
			auto find = [&](uint32_t x)
			{
				while (parent[x] != x) x = parent[x] = parent[parent[x]];
				return x;
			};

			for (uint32_t e0 : links.firstEvent)
			{
				if (e0 == 0 || e0 >= t.events) throw std::runtime_error("link table: a row's first event lies outside the event table");
				const uint32_t a = find(rowOfEvent[e0 - 1]), b = find(rowOfEvent[e0]);
				if (a != b) parent[std::max(a, b)] = std::min(a, b);
			}

			// ids ascend by root: a root is met before every other row of its component
			out.component.assign(rows, 0);
			for (size_t r = 0; r < rows; r++)
			{
				const uint32_t root = find(uint32_t(r));
				if (root == r)
				{
					out.component[r] = uint32_t(out.root.size());
					out.root.push_back(uint32_t(r));
				}
				else out.component[r] = out.component[root];
			}

			const size_t n = out.Rows();
			out.segments.assign(n, 0);
			out.links.assign(n, 0);
			out.length.assign(n, 0);
			out.edges.assign(n, 0);
			out.occurrences.assign(n, 0);
			out.presence.assign(n * words, 0);
			for (size_t r = 0; r < rows; r++)
			{
				const uint32_t p = out.component[r], e0 = colors.firstEvent[r];
				if (e0 >= t.events) throw std::runtime_error("colour table: a row's first event lies outside the event table");
				out.segments[p] += 1;
				out.length[p] += uint64_t(t.end[e0]) - t.begin[e0] + k;
				out.edges[p] += uint64_t(t.end[e0]) - t.begin[e0];
				out.occurrences[p] += colors.occurrences[r];
				for (size_t w = 0; w < words; w++) out.presence[p * words + w] |= colors.presence[r * words + w];
			}

			for (uint32_t e0 : links.firstEvent) out.links[out.component[rowOfEvent[e0]]] += 1;
		}

		namespace
		{
			void CheckComponents(const EventTable & t, const ColorTable & colors, const ComponentTable & c)
			{
				const size_t rows = colors.Rows(), words = colors.Words(), n = c.Rows();
				if (c.component.size() != rows || c.segments.size() != n || c.links.size() != n || c.length.size() != n || c.edges.size() != n || c.occurrences.size() != n ||
					c.presence.size() != n * words)
				{
					throw std::runtime_error("component table: the arrays do not agree about the rows, the components and the colours");
				}

				for (uint32_t e0 : colors.firstEvent)
				{
					if (e0 >= t.events) throw std::runtime_error("colour table: a row's first event lies outside the event table");
				}

				for (uint32_t p : c.component)
				{
					if (p >= n) throw std::runtime_error("component table: a row lies in no component");
				}

				for (uint32_t r : c.root)
				{
					if (r >= rows) throw std::runtime_error("component table: a root lies outside the segments");
				}
			}

			// the text `lines` appends to, written whenever it has grown past 1 MiB and at the end
			void WriteStreamed(const std::string & path, const char * what, const std::function<void(std::string & buf, const std::function<void()> & flushIfLarge)> & lines)
			{
				std::FILE * f = path.empty() ? stdout : std::fopen(path.c_str(), "wb");
				if (!f) throw std::runtime_error(std::string("Can't create the ") + what + " " + path);
				std::string buf;
				bool good = true;
				auto flush = [&]() { good = good && std::fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); };
				lines(buf, [&]() { if (buf.size() > (size_t(1) << 20)) flush(); });
				flush();
				good = good && std::fflush(f) == 0;
				if (f != stdout) good = (std::fclose(f) == 0) && good;
				if (!good)
				{
					if (f != stdout) ::unlink(path.c_str());
					throw std::runtime_error(std::string("Can't write the ") + what);
				}
			}
		}

		void WriteComponents(const EventTable & t, size_t k, const ColorMap & map, const ColorTable & colors, uint64_t links, const ComponentTable & c, const std::string & path)
		{
			CheckComponents(t, colors, c);
			if (map.label.size() != colors.colors) throw std::runtime_error("colour table: the arrays do not agree about the rows and the colours");
			const size_t words = colors.Words(), n = c.Rows(), digits = size_t((colors.colors + 3) / 4);
			// components and their segments by floor(log2(segments)): computed here from the rows, whichever source they have
			uint64_t sizeComponents[64] = {0}, sizeSegments[64] = {0};
			for (uint64_t s : c.segments)
			{
				if (s == 0) throw std::runtime_error("component table: a component holds no segment");
				const int b = 63 - __builtin_clzll(static_cast<unsigned long long>(s));
				sizeComponents[b] += 1;
				sizeSegments[b] += s;
			}

			WriteStreamed(path, "component table", [&](std::string & buf, const std::function<void()> & flushIfLarge)
			{
				buf += "#twopaco-components\t1\tby=" + std::string(map.bySequence ? "sequence" : "file") + "\tk=" + std::to_string(k) + "\tcolors=" + std::to_string(colors.colors) +
					"\tsegments=" + std::to_string(colors.Rows()) + "\tlinks=" + std::to_string(links) + "\tcomponents=" + std::to_string(n) + "\n";
				for (uint64_t col = 0; col < colors.colors; col++) buf += "#color\t" + std::to_string(col) + "\t" + map.label[col] + "\n";
				for (int b = 0; b < 64; b++)
				{
					if (sizeComponents[b]) buf += "#size\t" + std::to_string(b) + "\t" + std::to_string(sizeComponents[b]) + "\t" + std::to_string(sizeSegments[b]) + "\n";
				}

				for (size_t p = 0; p < n; p++)
				{
					buf += std::to_string(p);
					buf += '\t';
					buf += std::to_string(static_cast<long long>(Magnitude(t.name[colors.firstEvent[c.root[p]]])));
					for (uint64_t value : {c.segments[p], c.links[p], c.length[p], c.edges[p], c.occurrences[p]})
					{
						buf += '\t';
						buf += std::to_string(value);
					}

					const uint32_t * bits = &c.presence[p * words];
					uint32_t held = 0;
					for (size_t w = 0; w < words; w++) held += uint32_t(__builtin_popcount(bits[w]));
					buf += '\t';
					buf += std::to_string(held);
					buf += '\t';
					for (size_t j = 0; j < digits; j++) buf += "0123456789abcdef"[(bits[j >> 3] >> (4 * (j & 7))) & 15u];
					buf += '\n';
					flushIfLarge();
				}
			});
		}

		void WriteComponentMembers(const EventTable & t, size_t k, const ColorTable & colors, const ComponentTable & c, const std::string & path)
		{
			CheckComponents(t, colors, c);
			if (path.empty()) throw std::runtime_error("The component members need a file name");
			WriteStreamed(path, "component members", [&](std::string & buf, const std::function<void()> & flushIfLarge)
			{
				buf += "#twopaco-component-members\t1\tk=" + std::to_string(k) + "\tsegments=" + std::to_string(colors.Rows()) + "\tcomponents=" + std::to_string(c.Rows()) + "\n";
				for (size_t r = 0; r < colors.Rows(); r++)
				{
					buf += std::to_string(static_cast<long long>(Magnitude(t.name[colors.firstEvent[r]])));
					buf += '\t';
					buf += std::to_string(c.component[r]);
					buf += '\n';
					flushIfLarge();
				}
			});
		}

		void WriteComponentFiles(const EventTable & t, size_t k, const ColorMap & map, const ColorTable & colors, uint64_t links, const ComponentTable & c,
			const std::string & path, const std::string & membersPath)
		{
			if (!membersPath.empty()) WriteComponentMembers(t, k, colors, c, membersPath);
			try
			{
				WriteComponents(t, k, map, colors, links, c, path);
			}
			catch (...)
			{
				if (!membersPath.empty()) ::unlink(membersPath.c_str());
				throw;
			}
		}

		void ComputeClasses(const EventTable & t, size_t k, const ColorTable & colors, ClassTable & out)
		{
			const size_t rows = colors.Rows(), words = colors.Words();
			if (colors.occurrences.size() != rows || colors.presence.size() != rows * words) throw std::runtime_error("colour table: the arrays do not agree about the rows and the colours");
			out = ClassTable();
			out.classOf.resize(rows);
			std::map<std::vector<uint32_t>, uint32_t> classOfKey;
			for (size_t r = 0; r < rows; r++)
			{
				const uint32_t e0 = colors.firstEvent[r];
				if (e0 >= t.events) throw std::runtime_error("colour table: a row's first event lies outside the event table");
				const std::vector<uint32_t> key(colors.presence.begin() + r * words, colors.presence.begin() + (r + 1) * words);
				// rows come in ascending order: a key's first row opens its class, so the ids ascend by first
				const std::pair<std::map<std::vector<uint32_t>, uint32_t>::iterator, bool> at = classOfKey.insert(std::make_pair(key, uint32_t(out.first.size())));
				if (at.second)
				{
					out.first.push_back(uint32_t(r));
					out.segments.push_back(0);
					out.length.push_back(0);
					out.edges.push_back(0);
					out.occurrences.push_back(0);
					out.presence.insert(out.presence.end(), key.begin(), key.end());
				}

				const uint32_t p = at.first->second;
				const uint64_t weight = uint64_t(t.end[e0]) - t.begin[e0];
				out.classOf[r] = p;
				out.segments[p] += 1;
				out.length[p] += weight + k;
				out.edges[p] += weight;
				out.occurrences[p] += colors.occurrences[r];
			}
		}

		namespace
		{
			void CheckClasses(const EventTable & t, const ColorTable & colors, const ClassTable & c)
			{
				const size_t rows = colors.Rows(), words = colors.Words(), n = c.Rows();
				if (c.classOf.size() != rows || c.segments.size() != n || c.length.size() != n || c.edges.size() != n || c.occurrences.size() != n || c.presence.size() != n * words)
				{
					throw std::runtime_error("class table: the arrays do not agree about the rows, the classes and the colours");
				}

				for (uint32_t e0 : colors.firstEvent)
				{
					if (e0 >= t.events) throw std::runtime_error("colour table: a row's first event lies outside the event table");
				}

				for (uint32_t p : c.classOf)
				{
					if (p >= n) throw std::runtime_error("class table: a row lies in no class");
				}

				for (uint32_t r : c.first)
				{
					if (r >= rows) throw std::runtime_error("class table: a first row lies outside the segments");
				}
			}
		}

		void WriteClasses(const EventTable & t, size_t k, const ColorMap & map, const ColorTable & colors, const ClassTable & c, const std::string & path)
		{
			CheckClasses(t, colors, c);
			if (map.label.size() != colors.colors) throw std::runtime_error("colour table: the arrays do not agree about the rows and the colours");
			const size_t words = colors.Words(), n = c.Rows(), digits = size_t((colors.colors + 3) / 4);
			// classes, segments and edges by number of colours: computed here from the rows, whichever source they have
			std::vector<uint32_t> held(n, 0);
			std::vector<uint64_t> setClasses(colors.colors + 1, 0), setSegments(colors.colors + 1, 0), setEdges(colors.colors + 1, 0);
			for (size_t p = 0; p < n; p++)
			{
				if (c.segments[p] == 0) throw std::runtime_error("class table: a class holds no segment");
				for (size_t w = 0; w < words; w++) held[p] += uint32_t(__builtin_popcount(c.presence[p * words + w]));
				if (held[p] > colors.colors) throw std::runtime_error("class table: a class holds more colours than there are");
				setClasses[held[p]] += 1;
				setSegments[held[p]] += c.segments[p];
				setEdges[held[p]] += c.edges[p];
			}

			WriteStreamed(path, "class table", [&](std::string & buf, const std::function<void()> & flushIfLarge)
			{
				buf += "#twopaco-classes\t1\tby=" + std::string(map.bySequence ? "sequence" : "file") + "\tk=" + std::to_string(k) + "\tcolors=" + std::to_string(colors.colors) +
					"\tsegments=" + std::to_string(colors.Rows()) + "\tclasses=" + std::to_string(n) + "\n";
				for (uint64_t col = 0; col < colors.colors; col++) buf += "#color\t" + std::to_string(col) + "\t" + map.label[col] + "\n";
				for (uint64_t held_n = 0; held_n <= colors.colors; held_n++)
				{
					if (setClasses[held_n])
					{
						buf += "#sets\t" + std::to_string(held_n) + "\t" + std::to_string(setClasses[held_n]) + "\t" + std::to_string(setSegments[held_n]) + "\t" + std::to_string(setEdges[held_n]) + "\n";
					}
				}

				for (size_t p = 0; p < n; p++)
				{
					buf += std::to_string(p);
					buf += '\t';
					buf += std::to_string(static_cast<long long>(Magnitude(t.name[colors.firstEvent[c.first[p]]])));
					for (uint64_t value : {c.segments[p], c.length[p], c.edges[p], c.occurrences[p], uint64_t(held[p])})
					{
						buf += '\t';
						buf += std::to_string(value);
					}

					const uint32_t * bits = &c.presence[p * words];
					buf += '\t';
					for (size_t j = 0; j < digits; j++) buf += "0123456789abcdef"[(bits[j >> 3] >> (4 * (j & 7))) & 15u];
					buf += '\n';
					flushIfLarge();
				}
			});
		}

		void WriteClassMembers(const EventTable & t, size_t k, const ColorTable & colors, const ClassTable & c, const std::string & path)
		{
			CheckClasses(t, colors, c);
			if (path.empty()) throw std::runtime_error("The class members need a file name");
			WriteStreamed(path, "class members", [&](std::string & buf, const std::function<void()> & flushIfLarge)
			{
				buf += "#twopaco-class-members\t1\tk=" + std::to_string(k) + "\tsegments=" + std::to_string(colors.Rows()) + "\tclasses=" + std::to_string(c.Rows()) + "\n";
				for (size_t r = 0; r < colors.Rows(); r++)
				{
					buf += std::to_string(static_cast<long long>(Magnitude(t.name[colors.firstEvent[r]])));
					buf += '\t';
					buf += std::to_string(c.classOf[r]);
					buf += '\n';
					flushIfLarge();
				}
			});
		}

		void WriteClassFiles(const EventTable & t, size_t k, const ColorMap & map, const ColorTable & colors, const ClassTable & c, const std::string & path,
			const std::string & membersPath)
		{
			if (!membersPath.empty()) WriteClassMembers(t, k, colors, c, membersPath);
			try
			{
				WriteClasses(t, k, map, colors, c, path);
			}
			catch (...)
			{
				if (!membersPath.empty()) ::unlink(membersPath.c_str());
				throw;
			}
		}

		void ComputeTracks(const EventTable & t, size_t k, const std::vector<uint32_t> & colorOfSequence, uint64_t nColors, const ColorTable & colors, uint32_t only,
			TrackTable & out)
		{
			(void)k;
			const uint32_t ALL = TrackTable::ALL;
			if (nColors == 0) throw std::runtime_error("track table: at least one colour is required");
			if (only != ALL && only >= nColors) throw std::runtime_error("track table: the one colour is " + std::to_string(only) + ", there are " + std::to_string(nColors) + " colours");
			if (colorOfSequence.size() != t.sequences) throw std::runtime_error("track table: the colour of every sequence is required");
			for (uint32_t c : colorOfSequence)
			{
				if (c >= nColors) throw std::runtime_error("track table: a sequence has the colour " + std::to_string(c) + ", there are " + std::to_string(nColors) + " colours");
			}

			if (!t.seqEventBegin || t.seqEventBegin[0] != 0 || t.seqEventBegin[t.sequences] != t.events) throw std::runtime_error("event table: the sequences' event ranges do not cover the events");
			const size_t rows = colors.Rows(), words = colors.Words();
			if (colors.colors != nColors || colors.nColors.size() != rows || colors.presence.size() != rows * words) throw std::runtime_error("colour table: the arrays do not agree about the rows and the colours");
			out = TrackTable();
			out.colors = nColors;
			out.segments = rows;
			out.only = only;
			out.intervals.assign(nColors, 0);
			out.edges.assign(nColors, 0);
			out.coreEdges.assign(nColors, 0);
			out.privateEdges.assign(nColors, 0);
			out.depthIntervals.assign(nColors + 1, 0);
			out.depthEdges.assign(nColors + 1, 0);
			const int64_t FRESH = int64_t(1) << 34;
			std::unordered_map<int64_t, uint32_t> rowOf;
			uint32_t seen = 0, rowBefore = 0;
			size_t sequence = 0;
			auto close = [&]()
			{
				// the sums of the interval that ends at out.lastEvent.back()
				const uint32_t first = out.firstEvent.back(), last = out.lastEvent.back(), n = colors.nColors[out.row.back()];
				const uint32_t c = colorOfSequence[sequence];
				const uint64_t edges = uint64_t(t.end[last]) - t.begin[first];
				if (n > nColors) throw std::runtime_error("colour table: a row holds more colours than there are");
				out.intervals[c] += 1;
				out.edges[c] += edges;
				if (n == nColors) out.coreEdges[c] += edges;
				if (n == 1) out.privateEdges[c] += edges;
				out.depthIntervals[n] += 1;
				out.depthEdges[n] += edges;
			};

			bool open = false;
			for (uint64_t e = 0; e < t.events; e++)
			{
				bool begins = false;
				while (e >= t.seqEventBegin[sequence + 1])
				{
					if (open) close();
					open = false;
					++sequence;
					begins = true;
				}

				const int64_t name = Magnitude(t.name[e]);
				std::unordered_map<int64_t, uint32_t>::const_iterator at = name >= FRESH ? rowOf.end() : rowOf.find(name);
				uint32_t row = 0;
				if (at == rowOf.end())
				{
					row = seen++;
					if (name < FRESH) rowOf[name] = row;
				}
				else row = at->second;

				if (row >= rows) throw std::runtime_error("track table: the colour table holds fewer rows than the events have segments");
				const bool selected = only == ALL || colorOfSequence[sequence] == only;
				if (selected)
				{
					const bool continues = open && !begins && std::equal(colors.presence.begin() + size_t(row) * words, colors.presence.begin() + size_t(row + 1) * words,
						colors.presence.begin() + size_t(rowBefore) * words);
					if (continues) out.lastEvent.back() = uint32_t(e);
					else
					{
						if (open) close();
						out.firstEvent.push_back(uint32_t(e));
						out.lastEvent.push_back(uint32_t(e));
						out.row.push_back(row);
						open = true;
					}
				}

				rowBefore = row;
			}

			if (open) close();
		}

		namespace
		{
			// one interval as the writers print it
			struct TrackLine
			{
				uint32_t sequence, nColors;
				uint64_t begin, end, events;
			};

			void CheckTracks(const EventTable & t, const ColorMap & map, const InputSequences & seq, const ColorTable & colors, const TrackTable & a)
			{
				const size_t n = a.Rows();
				if (a.lastEvent.size() != n || a.row.size() != n || a.intervals.size() != a.colors || a.edges.size() != a.colors || a.coreEdges.size() != a.colors ||
					a.privateEdges.size() != a.colors || a.depthIntervals.size() != a.colors + 1 || a.depthEdges.size() != a.colors + 1 || map.label.size() != a.colors ||
					colors.colors != a.colors || (a.only != TrackTable::ALL && a.only >= a.colors))
				{
					throw std::runtime_error("track table: the arrays do not agree about the intervals and the colours");
				}

				if (colors.nColors.size() != colors.Rows() || colors.presence.size() != colors.Rows() * colors.Words()) throw std::runtime_error("colour table: the arrays do not agree about the rows and the colours");
				if (map.colorOfSequence.size() != t.sequences || seq.name.size() != t.sequences || seq.length.size() != t.sequences)
				{
					throw std::runtime_error("track table: the colour, the name and the length of every sequence are required");
				}

				if (!t.seqEventBegin || t.seqEventBegin[0] != 0 || t.seqEventBegin[t.sequences] != t.events) throw std::runtime_error("event table: the sequences' event ranges do not cover the events");
				for (size_t i = 0; i < n; i++)
				{
					if (a.firstEvent[i] > a.lastEvent[i] || a.lastEvent[i] >= t.events || a.row[i] >= colors.Rows() || t.end[a.lastEvent[i]] < t.begin[a.firstEvent[i]])
					{
						throw std::runtime_error("track table: an interval lies outside the event table");
					}
				}
			}

			TrackLine MakeTrackLine(const EventTable & t, const ColorTable & colors, const TrackTable & a, size_t i)
			{
				TrackLine line;
				const uint32_t first = a.firstEvent[i], last = a.lastEvent[i];
				line.sequence = uint32_t(std::upper_bound(t.seqEventBegin, t.seqEventBegin + t.sequences + 1, first) - t.seqEventBegin - 1);
				line.begin = t.begin[first];
				line.end = t.end[last];
				line.events = uint64_t(last) - first + 1;
				line.nColors = colors.nColors[a.row[i]];
				return line;
			}
		}

		void WriteTracks(const EventTable & t, size_t k, const ColorMap & map, const InputSequences & seq, const ColorTable & colors, const TrackTable & a, const std::string & path)
		{
			CheckTracks(t, map, seq, colors, a);
			const size_t words = colors.Words(), digits = size_t((colors.colors + 3) / 4);
			WriteStreamed(path, "track table", [&](std::string & buf, const std::function<void()> & flushIfLarge)
			{
				buf += "#twopaco-tracks\t1\tby=" + std::string(map.bySequence ? "sequence" : "file") + "\tk=" + std::to_string(k) + "\tcolors=" + std::to_string(a.colors) +
					"\tsegments=" + std::to_string(a.segments) + "\tof=" + (a.only == TrackTable::ALL ? std::string("all") : std::to_string(a.only)) + "\tintervals=" +
					std::to_string(a.Rows()) + "\n";
				for (uint64_t c = 0; c < a.colors; c++) buf += "#color\t" + std::to_string(c) + "\t" + map.label[c] + "\n";
				for (size_t s = 0; s < seq.name.size(); s++)
				{
					buf += "#sequence\t" + std::to_string(s) + "\t" + std::to_string(map.colorOfSequence[s]) + "\t" + std::to_string(seq.length[s]) + "\t" + seq.name[s] + "\n";
					flushIfLarge();
				}

				for (uint64_t c = 0; c < a.colors; c++)
				{
					if (a.only != TrackTable::ALL && c != a.only) continue;
					buf += "#genome\t" + std::to_string(c) + "\t" + std::to_string(a.intervals[c]) + "\t" + std::to_string(a.edges[c]) + "\t" + std::to_string(a.coreEdges[c]) + "\t" +
						std::to_string(a.privateEdges[c]) + "\n";
				}

				for (uint64_t n = 0; n <= a.colors; n++)
				{
					if (a.depthIntervals[n]) buf += "#depth\t" + std::to_string(n) + "\t" + std::to_string(a.depthIntervals[n]) + "\t" + std::to_string(a.depthEdges[n]) + "\n";
				}

				for (size_t i = 0; i < a.Rows(); i++)
				{
					const TrackLine line = MakeTrackLine(t, colors, a, i);
					buf += std::to_string(line.sequence) + "\t" + std::to_string(line.begin) + "\t" + std::to_string(line.end) + "\t" + std::to_string(line.events) + "\t" +
						std::to_string(line.nColors) + "\t";
					const uint32_t * bits = &colors.presence[size_t(a.row[i]) * words];
					for (size_t j = 0; j < digits; j++) buf += "0123456789abcdef"[(bits[j >> 3] >> (4 * (j & 7))) & 15u];
					buf += '\n';
					flushIfLarge();
				}
			});
		}

		void WriteTracksBedGraph(const EventTable & t, size_t k, const ColorMap & map, const InputSequences & seq, const ColorTable & colors, const TrackTable & a,
			const std::string & path)
		{
			CheckTracks(t, map, seq, colors, a);
			if (path.empty()) throw std::runtime_error("The track bedGraph needs a file name");
			WriteStreamed(path, "track bedGraph", [&](std::string & buf, const std::function<void()> & flushIfLarge)
			{
				buf += "track type=bedGraph name=\"n_colors\" description=\"twopaco tracks k=" + std::to_string(k) + " by=" + (map.bySequence ? "sequence" : "file") + "\"\n";
				for (size_t i = 0; i < a.Rows(); i++)
				{
					const TrackLine line = MakeTrackLine(t, colors, a, i);
					buf += seq.name[line.sequence] + "\t" + std::to_string(line.begin) + "\t" + std::to_string(line.end) + "\t" + std::to_string(line.nColors) + "\n";
					flushIfLarge();
				}
			});
		}

		void WriteTrackFiles(const EventTable & t, size_t k, const ColorMap & map, const InputSequences & seq, const ColorTable & colors, const TrackTable & a, const std::string & path,
			const std::string & bedGraphPath)
		{
			if (!bedGraphPath.empty()) WriteTracksBedGraph(t, k, map, seq, colors, a, bedGraphPath);
			try
			{
				WriteTracks(t, k, map, seq, colors, a, path);
			}
			catch (...)
			{
				if (!bedGraphPath.empty()) ::unlink(bedGraphPath.c_str());
				throw;
			}
		}

		void ComputeSuperbubbles(const EventTable & t, size_t k, const LinkTable & links, const ColorTable & colors, uint32_t maxInside, SuperbubbleTable & out)
		{
			(void)k;
			out = SuperbubbleTable();
			if (maxInside < 2 || maxInside > 62) throw std::runtime_error("superbubble table: max_inside = " + std::to_string(maxInside) + ", allowed are 2 .. 62");
			out.maxInside = maxInside;
			const size_t words = colors.Words();
			if (colors.presence.size() != colors.Rows() * words) throw std::runtime_error("colour table: the arrays do not agree about the rows and the colours");
			// the row of every segment: the order of the first sights, as ComputeColors numbers them
			const int64_t FRESH = int64_t(1) << 34;
			std::unordered_map<int64_t, uint32_t> rowOf;
			std::vector<uint32_t> rowOfEvent(size_t(t.events), 0);
			uint64_t rows = 0;
			for (uint64_t e = 0; e < t.events; e++)
			{
				const int64_t name = Magnitude(t.name[e]);
				std::unordered_map<int64_t, uint32_t>::const_iterator seen = name >= FRESH ? rowOf.end() : rowOf.find(name);
				if (seen == rowOf.end())
				{
					if (name < FRESH) rowOf[name] = uint32_t(rows);
					rowOfEvent[e] = uint32_t(rows++);
				}
				else rowOfEvent[e] = seen->second;
			}

			if (rows != colors.Rows()) throw std::runtime_error("superbubble table: the colour table's rows are not the segments of the event table");
			if (rows >= (uint64_t(1) << 31)) throw std::runtime_error("superbubble table: " + std::to_string(rows) + " segments, a side holds at most 2147483647");
			out.sides = 2 * rows;
			auto side = [&](uint64_t e) { return uint32_t(rowOfEvent[e] << 1 | (t.name[e] < 0 ? 1u : 0u)); };
			auto rev = [](uint32_t code) { return code ^ 1u; };
			std::vector<std::set<uint32_t> > outSet(size_t(out.sides));
			for (uint32_t e0 : links.firstEvent)
			{
				if (e0 == 0 || e0 >= t.events) throw std::runtime_error("link table: a row's first event lies outside the event table");
				const uint32_t from = side(e0 - 1), to = side(e0);
				outSet[from].insert(to);
				outSet[rev(to)].insert(rev(from));   // the same arc once more when the link is its own reverse: a set holds it once
			}

			for (const std::set<uint32_t> & heads : outSet) out.arcs += heads.size();
			for (uint32_t e0 : colors.firstEvent)
			{
				if (e0 >= t.events) throw std::runtime_error("colour table: a row's first event lies outside the event table");
			}

			const uint32_t NONE = 0xFFFFFFFFu;
			// the walk from s: the sides seen in `list`, those visited in `order` (a topological order of U without the exit); the exit or NONE
			std::vector<uint32_t> list, pending, order;
			std::vector<bool> visited;
			auto walk = [&](uint32_t s) -> uint32_t
			{
				list.assign(1, s);
				pending.assign(1, 0);
				visited.assign(1, false);
				order.clear();
				if (outSet[s].size() < 2) return NONE;
				std::vector<size_t> ready(1, 0);
				while (!ready.empty())
				{
					const size_t i = ready.back();
					ready.pop_back();
					visited[i] = true;
					order.push_back(uint32_t(i));
					const uint32_t v = list[i];
					if (outSet[v].empty()) return NONE;                                  // a dead end
					for (uint32_t u : outSet[v])
					{
						if (u == s) return NONE;                                         // an arc back to the entrance
						size_t j = list.size();
						for (size_t q = 0; q < list.size(); q++)
						{
							if (list[q] == rev(u)) return NONE;                          // both strands of a row
							if (list[q] == u) j = q;
						}

						if (j == list.size())
						{
							if (list.size() == size_t(maxInside) + 2) return NONE;      // one entry too many
							list.push_back(u);
							pending.push_back(uint32_t(outSet[rev(u)].size()));          // in(u) = rev(out(rev(u)))
							visited.push_back(false);
						}

						if (visited[j] || pending[j] == 0) return NONE;
						if (--pending[j] == 0) ready.push_back(j);
					}

					if (list.size() - order.size() == 1 && ready.size() == 1)            // one side left, and all its in-neighbours visited
					{
						const uint32_t exit = list[ready[0]];
						return outSet[exit].count(s) ? NONE : exit;                      // an arc from exit to entrance closes a cycle
					}
				}

				return NONE;   // sides are seen that wait for an in-neighbour outside: no matching
			};

			std::vector<uint32_t> exitOf(size_t(out.sides), NONE);
			for (uint64_t code = 0; code < out.sides; code++) exitOf[code] = walk(uint32_t(code));
			out.memberOffset.push_back(0);
			for (uint64_t code = 0; code < out.sides; code++)
			{
				const uint32_t s = uint32_t(code), exit = exitOf[code];
				if (exit == NONE) continue;
				const bool mirrored = exitOf[rev(exit)] == rev(s);
				if (!mirrored) out.unmirrored += 1;
				if (!(s < rev(exit) || !mirrored)) continue;
				if (walk(s) != exit) throw std::runtime_error("superbubble table: a walk did not repeat itself");
				const size_t n = list.size();
				std::vector<uint64_t> paths(n, 0), low(n, ~uint64_t(0)), high(n, 0);
				paths[0] = 1;
				low[0] = 0;
				uint32_t arcsIn = 0;
				for (uint32_t i : order)
				{
					arcsIn += uint32_t(outSet[list[i]].size());   // every arc that leaves a side of U other than the exit ends in U
					for (uint32_t u : outSet[list[i]])
					{
						const size_t j = size_t(std::find(list.begin(), list.end(), u) - list.begin());
						const uint32_t e0 = colors.firstEvent[u >> 1];
						const uint64_t weight = u == exit ? 0 : uint64_t(t.end[e0]) - t.begin[e0];
						paths[j] += paths[i];
						low[j] = std::min(low[j], low[i] + weight);
						high[j] = std::max(high[j], high[i] + weight);
					}
				}

				const size_t at = size_t(std::find(list.begin(), list.end(), exit) - list.begin());
				std::vector<uint32_t> inside;
				for (uint32_t u : list)
				{
					if (u != s && u != exit) inside.push_back(u);
				}

				std::sort(inside.begin(), inside.end());
				std::vector<uint32_t> bits(words, 0);
				for (uint32_t u : inside)
				{
					for (size_t w = 0; w < words; w++) bits[w] |= colors.presence[size_t(u >> 1) * words + w];
				}

				uint32_t held = 0;
				for (uint32_t w : bits) held += uint32_t(__builtin_popcount(w));
				out.entrance.push_back(s);
				out.exit.push_back(exit);
				out.inside.push_back(uint32_t(inside.size()));
				out.arcsIn.push_back(arcsIn);
				out.nColors.push_back(held);
				out.paths.push_back(paths[at]);
				out.minEdges.push_back(low[at]);
				out.maxEdges.push_back(high[at]);
				out.presence.insert(out.presence.end(), bits.begin(), bits.end());
				out.members.insert(out.members.end(), inside.begin(), inside.end());
				out.memberOffset.push_back(uint32_t(out.members.size()));
			}
		}

		namespace
		{
			void CheckSuperbubbles(const EventTable & t, const ColorTable & colors, const SuperbubbleTable & b)
			{
				const size_t n = b.Rows(), words = colors.Words();
				if (b.exit.size() != n || b.inside.size() != n || b.arcsIn.size() != n || b.nColors.size() != n || b.paths.size() != n || b.minEdges.size() != n ||
					b.maxEdges.size() != n || b.presence.size() != n * words || b.memberOffset.size() != n + 1 || b.memberOffset[0] != 0 || b.memberOffset[n] != b.members.size())
				{
					throw std::runtime_error("superbubble table: the arrays do not agree about the rows, the members and the colours");
				}

				if (b.sides != 2 * uint64_t(colors.Rows())) throw std::runtime_error("superbubble table: its sides are not those of the colour table's rows");
				for (uint32_t e0 : colors.firstEvent)
				{
					if (e0 >= t.events) throw std::runtime_error("colour table: a row's first event lies outside the event table");
				}

				for (const std::vector<uint32_t> * codes : {&b.entrance, &b.exit, &b.members})
				{
					for (uint32_t code : *codes)
					{
						if (code >= b.sides) throw std::runtime_error("superbubble table: a side lies outside the segments");
					}
				}

				for (size_t r = 0; r < n; r++)
				{
					if (b.memberOffset[r + 1] < b.memberOffset[r] || b.memberOffset[r + 1] - b.memberOffset[r] != b.inside[r] || b.inside[r] > b.maxInside)
					{
						throw std::runtime_error("superbubble table: a row's members are not its inside");
					}
				}
			}

			void AppendSide(std::string & buf, const EventTable & t, const ColorTable & colors, uint32_t code)
			{
				buf += std::to_string(static_cast<long long>(Magnitude(t.name[colors.firstEvent[code >> 1]])));
				buf += '\t';
				buf += (code & 1u) ? '-' : '+';
			}
		}

		void WriteSuperbubbles(const EventTable & t, size_t k, const ColorMap & map, const ColorTable & colors, uint64_t links, const SuperbubbleTable & b, const std::string & path)
		{
			CheckSuperbubbles(t, colors, b);
			if (map.label.size() != colors.colors) throw std::runtime_error("colour table: the arrays do not agree about the rows and the colours");
			const size_t words = colors.Words(), n = b.Rows(), digits = size_t((colors.colors + 3) / 4);
			uint64_t bySize[63] = {0};
			for (uint32_t inside : b.inside) bySize[inside] += 1;
			WriteStreamed(path, "superbubble table", [&](std::string & buf, const std::function<void()> & flushIfLarge)
			{
				buf += "#twopaco-superbubbles\t1\tby=" + std::string(map.bySequence ? "sequence" : "file") + "\tk=" + std::to_string(k) + "\tcolors=" + std::to_string(colors.colors) +
					"\tsegments=" + std::to_string(colors.Rows()) + "\tlinks=" + std::to_string(links) + "\tmax_inside=" + std::to_string(b.maxInside) + "\tsuperbubbles=" +
					std::to_string(n) + "\n";
				for (uint64_t col = 0; col < colors.colors; col++) buf += "#color\t" + std::to_string(col) + "\t" + map.label[col] + "\n";
				for (int size = 0; size < 63; size++)
				{
					if (bySize[size]) buf += "#inside\t" + std::to_string(size) + "\t" + std::to_string(bySize[size]) + "\n";
				}

				for (size_t r = 0; r < n; r++)
				{
					AppendSide(buf, t, colors, b.entrance[r]);
					buf += '\t';
					AppendSide(buf, t, colors, b.exit[r]);
					for (uint64_t value : {uint64_t(b.inside[r]), uint64_t(b.arcsIn[r]), b.paths[r], b.minEdges[r], b.maxEdges[r], uint64_t(b.nColors[r])})
					{
						buf += '\t';
						buf += std::to_string(value);
					}

					const uint32_t * bits = &b.presence[r * words];
					buf += '\t';
					for (size_t j = 0; j < digits; j++) buf += "0123456789abcdef"[(bits[j >> 3] >> (4 * (j & 7))) & 15u];
					buf += '\n';
					flushIfLarge();
				}
			});
		}

		void WriteSuperbubbleMembers(const EventTable & t, size_t k, const ColorTable & colors, const SuperbubbleTable & b, const std::string & path)
		{
			CheckSuperbubbles(t, colors, b);
			if (path.empty()) throw std::runtime_error("The superbubble members need a file name");
			WriteStreamed(path, "superbubble members", [&](std::string & buf, const std::function<void()> & flushIfLarge)
			{
				buf += "#twopaco-superbubble-members\t1\tk=" + std::to_string(k) + "\tsegments=" + std::to_string(colors.Rows()) + "\tmax_inside=" + std::to_string(b.maxInside) +
					"\tsuperbubbles=" + std::to_string(b.Rows()) + "\tmembers=" + std::to_string(b.members.size()) + "\n";
				for (size_t r = 0; r < b.Rows(); r++)
				{
					for (uint32_t m = b.memberOffset[r]; m < b.memberOffset[r + 1]; m++)
					{
						buf += std::to_string(r);
						buf += '\t';
						AppendSide(buf, t, colors, b.members[m]);
						buf += '\n';
					}

					flushIfLarge();
				}
			});
		}

		void WriteSuperbubbleFiles(const EventTable & t, size_t k, const ColorMap & map, const ColorTable & colors, uint64_t links, const SuperbubbleTable & b,
			const std::string & path, const std::string & membersPath)
		{
			if (!membersPath.empty()) WriteSuperbubbleMembers(t, k, colors, b, membersPath);
			try
			{
				WriteSuperbubbles(t, k, map, colors, links, b, path);
			}
			catch (...)
			{
				if (!membersPath.empty()) ::unlink(membersPath.c_str());
				throw;
			}
		}

		void ComputeVariants(const EventTable & t, size_t k, const std::vector<uint32_t> & colorOfSequence, uint64_t nColors, const ColorTable & colors, const SuperbubbleTable & b,
			uint32_t ref, VariantTable & out)
		{
			(void)k;
			const uint32_t NONE = VariantTable::NONE;
			if (nColors == 0) throw std::runtime_error("variant table: at least one colour is required");
			if (ref != NONE && ref >= nColors) throw std::runtime_error("variant table: the reference colour is " + std::to_string(ref) + ", there are " + std::to_string(nColors) + " colours");
			if (colorOfSequence.size() != t.sequences) throw std::runtime_error("variant table: the colour of every sequence is required");
			for (uint32_t c : colorOfSequence)
			{
				if (c >= nColors) throw std::runtime_error("variant table: a sequence has the colour " + std::to_string(c) + ", there are " + std::to_string(nColors) + " colours");
			}

			if (!t.seqEventBegin || t.seqEventBegin[0] != 0 || t.seqEventBegin[t.sequences] != t.events) throw std::runtime_error("event table: the sequences' event ranges do not cover the events");
			CheckSuperbubbles(t, colors, b);
			const size_t rows = colors.Rows(), words = size_t((nColors + 31) / 32), nb = b.Rows();
			out = VariantTable();
			out.colors = nColors;
			out.segments = rows;
			out.ref = ref;
			// the side and the sequence of every event
			const int64_t FRESH = int64_t(1) << 34;
			std::unordered_map<int64_t, uint32_t> rowOf;
			std::vector<uint32_t> side(t.events), sequenceOf(t.events);
			uint32_t seen = 0;
			size_t sequence = 0;
			for (uint64_t e = 0; e < t.events; e++)
			{
				while (e >= t.seqEventBegin[sequence + 1]) ++sequence;
				const int64_t name = Magnitude(t.name[e]);
				std::unordered_map<int64_t, uint32_t>::const_iterator at = name >= FRESH ? rowOf.end() : rowOf.find(name);
				uint32_t row = 0;
				if (at == rowOf.end())
				{
					row = seen++;
					if (name < FRESH) rowOf[name] = row;
				}
				else row = at->second;

				if (row >= rows) throw std::runtime_error("variant table: the colour table holds fewer rows than the events have segments");
				side[e] = row * 2 + (t.name[e] < 0 ? 1u : 0u);
				sequenceOf[e] = uint32_t(sequence);
			}

			std::unordered_map<uint32_t, uint32_t> rowOfEntrance;
			for (size_t r = 0; r < nb; r++) rowOfEntrance[b.entrance[r]] = uint32_t(r);
			// both walks of every event
			for (uint64_t e = 0; e < t.events; e++)
			{
				for (uint32_t d = 0; d < 2; d++)
				{
					std::unordered_map<uint32_t, uint32_t>::const_iterator at = rowOfEntrance.find(side[e] ^ d);
					if (at == rowOfEntrance.end()) continue;
					const uint32_t r = at->second;
					const uint32_t * members = b.members.data() + b.memberOffset[r];
					const uint32_t inside = b.inside[r];
					const uint64_t lowest = t.seqEventBegin[sequenceOf[e]], beyond = t.seqEventBegin[sequenceOf[e] + 1];
					uint64_t mask = 0, x = e;
					bool reached = false;
					for (uint32_t step = 0; step <= b.maxInside && !reached; step++)
					{
						if (d ? x == lowest : x + 1 == beyond) break;   // the sequence ends inside the superbubble
						x = d ? x - 1 : x + 1;
						const uint32_t read = side[x] ^ d;
						if (read == b.exit[r]) { reached = true; break; }
						const uint32_t * m = std::lower_bound(members, members + inside, read);
						if (m == members + inside || *m != read) { out.strays += 1; break; }
						mask |= uint64_t(1) << (m - members);
					}

					if (!reached) continue;
					const uint64_t lo = std::min(e, x), hi = std::max(e, x);
					out.start.push_back(uint32_t(e));
					out.last.push_back(uint32_t(x));
					out.dir.push_back(d);
					out.row.push_back(r);
					out.mask.push_back(mask);
					out.edges.push_back(t.begin[hi] >= t.end[lo] ? t.begin[hi] - t.end[lo] : t.end[lo] - t.begin[hi]);
				}
			}

			// the alleles: (row, mask) -> its traversals, in the order (row, first)
			const size_t n = out.Traversals();
			std::map<std::pair<uint32_t, uint64_t>, uint32_t> found;   // -> first
			for (size_t i = 0; i < n; i++) found.insert(std::make_pair(std::make_pair(out.row[i], out.mask[i]), uint32_t(i)));
			std::vector<std::pair<uint32_t, uint32_t> > order;         // (row, first)
			for (const auto & f : found) order.push_back(std::make_pair(f.first.first, f.second));
			std::sort(order.begin(), order.end());
			const size_t alleles = order.size();
			std::map<std::pair<uint32_t, uint64_t>, uint32_t> alleleOf;
			out.alleleOffset.assign(nb + 1, 0);
			for (size_t a = 0; a < alleles; a++)
			{
				const uint32_t first = order[a].second;
				alleleOf[std::make_pair(out.row[first], out.mask[first])] = uint32_t(a);
				out.alleleRow.push_back(out.row[first]);
				out.alleleMask.push_back(out.mask[first]);
				out.sides.push_back(uint32_t(__builtin_popcountll(out.mask[first])));
				out.alleleEdges.push_back(out.edges[first]);
				out.first.push_back(first);
				out.alleleOffset[out.row[first] + 1] += 1;
			}

			for (size_t r = 0; r < nb; r++) out.alleleOffset[r + 1] += out.alleleOffset[r];
			out.traversals.assign(alleles, 0);
			out.nColors.assign(alleles, 0);
			out.presence.assign(alleles * words, 0);
			out.refAllele.assign(nb, NONE);
			out.siteTraversals.assign(nb, 0);
			out.refTraversals.assign(nb, 0);
			for (size_t i = 0; i < n; i++)
			{
				const uint32_t a = alleleOf[std::make_pair(out.row[i], out.mask[i])], c = colorOfSequence[sequenceOf[out.start[i]]], r = out.row[i];
				out.traversals[a] += 1;
				out.siteTraversals[r] += 1;
				out.presence[a * words + c / 32] |= 1u << (c % 32);
				if (c == ref)
				{
					if (out.refTraversals[r] == 0) out.refAllele[r] = a;
					out.refTraversals[r] += 1;
				}
			}

			for (size_t a = 0; a < alleles; a++)
			{
				for (size_t w = 0; w < words; w++) out.nColors[a] += uint32_t(__builtin_popcount(out.presence[a * words + w]));
			}
		}

		namespace
		{
			void CheckVariants(const EventTable & t, const ColorMap & map, const InputSequences & seq, const ColorTable & colors, const SuperbubbleTable & b, const VariantTable & v)
			{
				CheckSuperbubbles(t, colors, b);
				const size_t n = v.Traversals(), a = v.Alleles(), nb = b.Rows(), words = colors.Words();
				if (v.last.size() != n || v.dir.size() != n || v.row.size() != n || v.edges.size() != n || v.mask.size() != n || v.alleleRow.size() != a || v.sides.size() != a ||
					v.alleleEdges.size() != a || v.nColors.size() != a || v.alleleMask.size() != a || v.traversals.size() != a || v.presence.size() != a * words ||
					v.alleleOffset.size() != nb + 1 || v.alleleOffset[0] != 0 || v.alleleOffset[nb] != a || v.refAllele.size() != nb || v.siteTraversals.size() != nb ||
					v.refTraversals.size() != nb || map.label.size() != v.colors || colors.colors != v.colors || (v.ref != VariantTable::NONE && v.ref >= v.colors))
				{
					throw std::runtime_error("variant table: the arrays do not agree about the traversals, the alleles, the sites and the colours");
				}

				if (map.colorOfSequence.size() != t.sequences || seq.name.size() != t.sequences || seq.length.size() != t.sequences)
				{
					throw std::runtime_error("variant table: the colour, the name and the length of every sequence are required");
				}

				if (!t.seqEventBegin || t.seqEventBegin[0] != 0 || t.seqEventBegin[t.sequences] != t.events) throw std::runtime_error("event table: the sequences' event ranges do not cover the events");
				for (size_t i = 0; i < n; i++)
				{
					if (v.start[i] >= t.events || v.last[i] >= t.events || v.row[i] >= nb || v.dir[i] > 1) throw std::runtime_error("variant table: a traversal lies outside the tables");
				}

				for (size_t r = 0; r < nb; r++)
				{
					if (v.alleleOffset[r + 1] < v.alleleOffset[r] || (v.refAllele[r] != VariantTable::NONE && (v.refAllele[r] < v.alleleOffset[r] || v.refAllele[r] >= v.alleleOffset[r + 1])))
					{
						throw std::runtime_error("variant table: a site's alleles are not its own");
					}
				}

				for (size_t i = 0; i < a; i++)
				{
					if (v.first[i] >= n || v.alleleRow[i] >= nb) throw std::runtime_error("variant table: an allele lies outside the tables");
				}
			}

			// the span of traversal i: its sequence and the positions [begin, end) in bases
			struct VariantSpan
			{
				uint32_t sequence;
				uint64_t begin, end;
			};

			VariantSpan MakeVariantSpan(const EventTable & t, size_t k, const VariantTable & v, size_t i)
			{
				const uint32_t lo = std::min(v.start[i], v.last[i]), hi = std::max(v.start[i], v.last[i]);
				VariantSpan span;
				span.sequence = uint32_t(std::upper_bound(t.seqEventBegin, t.seqEventBegin + t.sequences + 1, lo) - t.seqEventBegin - 1);
				span.begin = t.end[lo];
				span.end = uint64_t(t.begin[hi]) + k;
				return span;
			}

			void AppendPresence(std::string & buf, const uint32_t * bits, size_t digits)
			{
				for (size_t j = 0; j < digits; j++) buf += "0123456789abcdef"[(bits[j >> 3] >> (4 * (j & 7))) & 15u];
			}

			// the letters of a span as stored, every letter other than A C G T an N
			std::string SpanLetters(const LoadedSequences & loaded, const VariantSpan & span)
			{
				if (span.sequence >= loaded.body.size() || span.end > loaded.body[span.sequence].size() || span.begin > span.end)
				{
					throw std::runtime_error("variant table: a traversal lies outside the letters of its sequence");
				}

				std::string s = loaded.body[span.sequence].substr(size_t(span.begin), size_t(span.end - span.begin));
				for (char & ch : s) if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') ch = 'N';
				return s;
			}

			std::string ReverseComplementN(const std::string & s)
			{
				std::string r(s.rbegin(), s.rend());
				for (char & ch : r) ch = ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : 'N';
				return r;
			}
		}

		void WriteVariants(const EventTable & t, size_t k, const ColorMap & map, const InputSequences & seq, const ColorTable & colors, const SuperbubbleTable & b,
			const VariantTable & v, const std::string & path)
		{
			CheckVariants(t, map, seq, colors, b, v);
			const size_t words = colors.Words(), digits = size_t((colors.colors + 3) / 4), nb = b.Rows();
			std::map<uint32_t, uint64_t> byAlleles;
			for (size_t r = 0; r < nb; r++) if (v.alleleOffset[r + 1] > v.alleleOffset[r]) byAlleles[v.alleleOffset[r + 1] - v.alleleOffset[r]] += 1;
			WriteStreamed(path, "variant table", [&](std::string & buf, const std::function<void()> & flushIfLarge)
			{
				buf += "#twopaco-variants\t1\tby=" + std::string(map.bySequence ? "sequence" : "file") + "\tk=" + std::to_string(k) + "\tcolors=" + std::to_string(v.colors) +
					"\tsegments=" + std::to_string(v.segments) + "\tsuperbubbles=" + std::to_string(nb) + "\tmax_inside=" + std::to_string(b.maxInside) + "\tref=" +
					(v.ref == VariantTable::NONE ? std::string("none") : std::to_string(v.ref)) + "\tsites=" + std::to_string(v.Sites()) + "\talleles=" + std::to_string(v.Alleles()) +
					"\ttraversals=" + std::to_string(v.Traversals()) + "\n";
				for (uint64_t c = 0; c < v.colors; c++) buf += "#color\t" + std::to_string(c) + "\t" + map.label[c] + "\n";
				for (size_t s = 0; s < seq.name.size(); s++)
				{
					buf += "#sequence\t" + std::to_string(s) + "\t" + std::to_string(map.colorOfSequence[s]) + "\t" + std::to_string(seq.length[s]) + "\t" + seq.name[s] + "\n";
					flushIfLarge();
				}

				for (const auto & bin : byAlleles) buf += "#alleles\t" + std::to_string(bin.first) + "\t" + std::to_string(bin.second) + "\n";
				for (size_t r = 0; r < nb; r++)
				{
					for (uint32_t a = v.alleleOffset[r]; a < v.alleleOffset[r + 1]; a++)
					{
						const VariantSpan span = MakeVariantSpan(t, k, v, v.first[a]);
						buf += std::to_string(r);
						buf += '\t';
						AppendSide(buf, t, colors, b.entrance[r]);
						buf += '\t';
						AppendSide(buf, t, colors, b.exit[r]);
						for (uint64_t value : {uint64_t(a - v.alleleOffset[r]), v.traversals[a], uint64_t(v.sides[a]), uint64_t(v.alleleEdges[a]), uint64_t(v.nColors[a])})
						{
							buf += '\t';
							buf += std::to_string(value);
						}

						buf += '\t';
						AppendPresence(buf, &v.presence[size_t(a) * words], digits);
						buf += "\t" + std::to_string(span.sequence) + "\t" + std::to_string(span.begin) + "\t" + std::to_string(span.end) + "\t" + (v.dir[v.first[a]] ? "-" : "+") + "\t" +
							(v.ref != VariantTable::NONE && v.refAllele[r] == a ? "1" : "0") + "\n";
					}

					flushIfLarge();
				}
			});
		}

		void WriteVariantsVcf(const EventTable & t, size_t k, const ColorMap & map, const InputSequences & seq, const LoadedSequences & loaded, const ColorTable & colors,
			const SuperbubbleTable & b, const VariantTable & v, const std::string & path)
		{
			CheckVariants(t, map, seq, colors, b, v);
			if (path.empty()) throw std::runtime_error("The variant VCF needs a file name");
			if (v.ref == VariantTable::NONE) throw std::runtime_error("The variant VCF needs a reference colour");
			if (k == 0) throw std::runtime_error("The variant VCF needs k above 0");
			const size_t words = colors.Words(), nb = b.Rows();
			// the reference traversal of every site: the smallest one that starts in the reference colour
			std::vector<uint32_t> refTraversal(nb, VariantTable::NONE);
			for (size_t i = v.Traversals(); i-- > 0;)
			{
				const VariantSpan span = MakeVariantSpan(t, k, v, i);
				if (map.colorOfSequence[span.sequence] == v.ref) refTraversal[v.row[i]] = uint32_t(i);
			}

			struct Record
			{
				uint32_t sequence, site;
				uint64_t pos;
				bool operator < (const Record & o) const { return sequence != o.sequence ? sequence < o.sequence : pos != o.pos ? pos < o.pos : site < o.site; }
			};

			std::vector<Record> records;
			for (size_t r = 0; r < nb; r++)
			{
				const uint32_t a0 = v.alleleOffset[r], a1 = v.alleleOffset[r + 1];
				if (refTraversal[r] == VariantTable::NONE || v.refAllele[r] == VariantTable::NONE || a1 - a0 < 2) continue;
				// (equal edges below k + 1 cannot be in a graph of all (k+1)-mers; under an abundance cut they are, and take the anchored form)
				bool equal = v.alleleEdges[a0] >= k + 1;
				for (uint32_t a = a0; a < a1; a++) equal = equal && v.alleleEdges[a] == v.alleleEdges[a0];
				const VariantSpan span = MakeVariantSpan(t, k, v, refTraversal[r]);
				const Record record = {span.sequence, uint32_t(r), span.begin + k + (equal ? 1 : 0)};
				records.push_back(record);
			}

			std::sort(records.begin(), records.end());
			WriteStreamed(path, "variant VCF", [&](std::string & buf, const std::function<void()> & flushIfLarge)
			{
				buf += "##fileformat=VCFv4.2\n##source=twopaco variants k=" + std::to_string(k) + " by=" + (map.bySequence ? "sequence" : "file") + " ref=" + std::to_string(v.ref) +
					" max_inside=" + std::to_string(b.maxInside) + "\n";
				for (size_t s = 0; s < seq.name.size(); s++)
				{
					if (map.colorOfSequence[s] == v.ref) buf += "##contig=<ID=" + seq.name[s] + ",length=" + std::to_string(seq.length[s]) + ">\n";
				}

				buf += "##INFO=<ID=AC,Number=A,Type=Integer,Description=\"Traversals of each ALT allele\">\n"
					"##INFO=<ID=AN,Number=1,Type=Integer,Description=\"Traversals of the site\">\n"
					"##INFO=<ID=NS,Number=1,Type=Integer,Description=\"Colours with a traversal of the site\">\n"
					"##INFO=<ID=INS,Number=1,Type=Integer,Description=\"Sides inside the superbubble\">\n"
					"##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Alleles the colour walks\">\n"
					"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT";
				for (const std::string & label : map.label)
				{
					buf += '\t';
					for (char ch : label) buf += static_cast<unsigned char>(ch) <= ' ' ? '_' : ch;
				}

				buf += '\n';
				for (const Record & record : records)
				{
					const size_t r = record.site;
					const uint32_t a0 = v.alleleOffset[r], a1 = v.alleleOffset[r + 1], refAllele = v.refAllele[r], refDir = v.dir[refTraversal[r]];
					// the record's alleles: the reference's first, then the others in allele order
					std::vector<uint32_t> local(1, refAllele);
					for (uint32_t a = a0; a < a1; a++) if (a != refAllele) local.push_back(a);
					uint32_t least = v.alleleEdges[a0];
					bool equal = v.alleleEdges[a0] >= k + 1;
					for (uint32_t a = a0; a < a1; a++)
					{
						equal = equal && v.alleleEdges[a] == v.alleleEdges[a0];
						least = std::min(least, v.alleleEdges[a]);
					}

					buf += seq.name[record.sequence] + "\t" + std::to_string(record.pos) + "\tsb" + std::to_string(r) + "\t";
					std::vector<uint32_t> present(words, 0);
					for (size_t i = 0; i < local.size(); i++)
					{
						const uint32_t a = local[i], from = i == 0 ? refTraversal[r] : v.first[a];
						std::string letters = SpanLetters(loaded, MakeVariantSpan(t, k, v, from));
						if (v.dir[from] != refDir) letters = ReverseComplementN(letters);
						const uint64_t edges = v.alleleEdges[a];
						if (letters.size() != edges + k) throw std::runtime_error("variant table: an allele's span is not its edges and k letters");
						const std::string text = equal ? letters.substr(k, size_t(edges - k)) : letters.substr(k - 1, size_t(edges + 1 - std::min<uint64_t>(k, least)));
						if (text.empty()) throw std::runtime_error("variant table: an allele of a record spells nothing");
						buf += text;
						buf += i == 0 ? '\t' : i + 1 < local.size() ? ',' : '\t';
						for (size_t w = 0; w < words; w++) present[w] |= v.presence[size_t(a) * words + w];
					}

					buf += ".\t.\tAC=";
					for (size_t i = 1; i < local.size(); i++) buf += std::to_string(v.traversals[local[i]]) + (i + 1 < local.size() ? "," : "");
					uint32_t ns = 0;
					for (uint32_t w : present) ns += uint32_t(__builtin_popcount(w));
					buf += ";AN=" + std::to_string(v.siteTraversals[r]) + ";NS=" + std::to_string(ns) + ";INS=" + std::to_string(b.inside[r]) + "\tGT";
					for (uint64_t c = 0; c < v.colors; c++)
					{
						std::string gt;
						for (size_t i = 0; i < local.size(); i++)
						{
							if (v.presence[size_t(local[i]) * words + c / 32] >> (c % 32) & 1u) gt += (gt.empty() ? "" : "/") + std::to_string(i);
						}

						buf += "\t" + (gt.empty() ? std::string(".") : gt);
					}

					buf += '\n';
					flushIfLarge();
				}
			});
		}

		void WriteVariantFiles(const EventTable & t, size_t k, const ColorMap & map, const InputSequences & seq, const LoadedSequences * loaded, const ColorTable & colors,
			const SuperbubbleTable & b, const VariantTable & v, const std::string & path, const std::string & vcfPath)
		{
			if (!vcfPath.empty())
			{
				if (!loaded) throw std::runtime_error("The variant VCF needs the letters of the input");
				WriteVariantsVcf(t, k, map, seq, *loaded, colors, b, v, vcfPath);
			}

			try
			{
				WriteVariants(t, k, map, seq, colors, b, v, path);
			}
			catch (...)
			{
				if (!vcfPath.empty()) ::unlink(vcfPath.c_str());
				throw;
			}
		}

		void ComputeAnchors(const EventTable & t, size_t k, const std::vector<uint32_t> & colorOfSequence, uint64_t colors, uint32_t ref, AnchorTable & out)
		{
			(void)k;
			if (colors == 0) throw std::runtime_error("anchor table: at least one colour is required");
			if (ref >= colors) throw std::runtime_error("anchor table: the reference colour is " + std::to_string(ref) + ", there are " + std::to_string(colors) + " colours");
			if (colorOfSequence.size() != t.sequences) throw std::runtime_error("anchor table: the colour of every sequence is required");
			for (uint32_t c : colorOfSequence)
			{
				if (c >= colors) throw std::runtime_error("anchor table: a sequence has the colour " + std::to_string(c) + ", there are " + std::to_string(colors) + " colours");
			}

			if (!t.seqEventBegin || t.seqEventBegin[0] != 0 || t.seqEventBegin[t.sequences] != t.events) throw std::runtime_error("event table: the sequences' event ranges do not cover the events");
			out = AnchorTable();
			out.colors = colors;
			out.ref = ref;
			const uint32_t NONE = AnchorTable::NONE;
			const int64_t FRESH = int64_t(1) << 34;
			// the row, the sequence and the colour of every event; count[row][colour] with the last event counted
			std::unordered_map<int64_t, uint32_t> rowOf;
			std::vector<uint32_t> rowOfEvent(size_t(t.events)), seqOfEvent(size_t(t.events));
			std::map<std::pair<uint32_t, uint32_t>, std::pair<uint64_t, uint32_t> > count;
			uint32_t sequence = 0;
			for (uint64_t e = 0; e < t.events; e++)
			{
				while (e >= t.seqEventBegin[sequence + 1]) ++sequence;
				const int64_t name = Magnitude(t.name[e]);
				std::unordered_map<int64_t, uint32_t>::const_iterator seen = name >= FRESH ? rowOf.end() : rowOf.find(name);
				if (seen == rowOf.end())
				{
					if (name < FRESH) rowOf[name] = uint32_t(out.segments);
					rowOfEvent[e] = uint32_t(out.segments++);
				}
				else rowOfEvent[e] = seen->second;

				seqOfEvent[e] = sequence;
				std::pair<uint64_t, uint32_t> & held = count[std::make_pair(rowOfEvent[e], colorOfSequence[sequence])];
				held.first += 1;
				held.second = uint32_t(e);
				if (colorOfSequence[sequence] == ref) out.refEdges += uint64_t(t.end[e]) - t.begin[e];
			}

			out.mate.assign(size_t(t.events), NONE);
			for (uint64_t e = 0; e < t.events; e++)
			{
				const uint32_t c = colorOfSequence[seqOfEvent[e]];
				if (c == ref || count[std::make_pair(rowOfEvent[e], c)].first != 1) continue;
				std::map<std::pair<uint32_t, uint32_t>, std::pair<uint64_t, uint32_t> >::const_iterator inRef = count.find(std::make_pair(rowOfEvent[e], ref));
				if (inRef != count.end() && inRef->second.first == 1) out.mate[e] = inRef->second.second;
			}

			auto reverse = [&](uint64_t e) { return (t.name[e] < 0) != (t.name[out.mate[e]] < 0); };
			auto continues = [&](uint64_t e)
			{
				if (e == 0 || out.mate[e] == NONE || out.mate[e - 1] == NONE || seqOfEvent[e] != seqOfEvent[e - 1] || reverse(e) != reverse(e - 1)) return false;
				const uint64_t m = out.mate[e], before = out.mate[e - 1];
				return (reverse(e) ? m + 1 == before : m == before + 1) && seqOfEvent[m] == seqOfEvent[before];
			};

			out.blocks.assign(colors, 0);
			out.anchors.assign(colors, 0);
			out.edges.assign(colors, 0);
			out.reverseEdges.assign(colors, 0);
			for (uint64_t e = 0; e < t.events; e++)
			{
				if (out.mate[e] == NONE || continues(e)) continue;
				uint64_t last = e;
				while (last + 1 < t.events && continues(last + 1)) ++last;
				const bool rev = reverse(e);
				out.queryFirst.push_back(uint32_t(e));
				out.queryLast.push_back(uint32_t(last));
				out.refFirst.push_back(rev ? out.mate[last] : out.mate[e]);
				out.refLast.push_back(rev ? out.mate[e] : out.mate[last]);
				const uint32_t c = colorOfSequence[seqOfEvent[e]];
				const uint64_t edges = uint64_t(t.end[last]) - t.begin[e];
				out.blocks[c] += 1;
				out.anchors[c] += last - e + 1;
				out.edges[c] += edges;
				if (rev) out.reverseEdges[c] += edges;
			}
		}

		namespace
		{
			// one block as the writers print it: colour, strand, and on each side the sequence and the half-open interval
			struct AnchorLine
			{
				uint32_t color, refSeq, querySeq;
				uint64_t refBegin, refEnd, queryBegin, queryEnd, anchors;
				bool reverse;
			};

			void CheckAnchors(const EventTable & t, const ColorMap & map, const InputSequences & seq, const AnchorTable & a)
			{
				const size_t n = a.Rows();
				if (a.queryLast.size() != n || a.refFirst.size() != n || a.refLast.size() != n || a.mate.size() != t.events || a.blocks.size() != a.colors ||
					a.anchors.size() != a.colors || a.edges.size() != a.colors || a.reverseEdges.size() != a.colors || map.label.size() != a.colors || a.ref >= a.colors)
				{
					throw std::runtime_error("anchor table: the arrays do not agree about the blocks, the events and the colours");
				}

				if (map.colorOfSequence.size() != t.sequences || seq.name.size() != t.sequences || seq.length.size() != t.sequences)
				{
					throw std::runtime_error("anchor table: the colour, the name and the length of every sequence are required");
				}

				if (!t.seqEventBegin || t.seqEventBegin[0] != 0 || t.seqEventBegin[t.sequences] != t.events) throw std::runtime_error("event table: the sequences' event ranges do not cover the events");
				for (size_t b = 0; b < n; b++)
				{
					if (a.queryFirst[b] > a.queryLast[b] || a.queryLast[b] >= t.events || a.refFirst[b] > a.refLast[b] || a.refLast[b] >= t.events ||
						a.refLast[b] - a.refFirst[b] != a.queryLast[b] - a.queryFirst[b] || a.mate[a.queryFirst[b]] >= t.events)
					{
						throw std::runtime_error("anchor table: a block lies outside the event table");
					}
				}
			}

			AnchorLine MakeAnchorLine(const EventTable & t, size_t k, const ColorMap & map, const AnchorTable & a, size_t b)
			{
				auto sequenceOf = [&](uint32_t e) { return uint32_t(std::upper_bound(t.seqEventBegin, t.seqEventBegin + t.sequences + 1, e) - t.seqEventBegin - 1); };
				AnchorLine line;
				const uint32_t qf = a.queryFirst[b], ql = a.queryLast[b], rf = a.refFirst[b], rl = a.refLast[b];
				line.querySeq = sequenceOf(qf);
				line.refSeq = sequenceOf(rf);
				line.color = map.colorOfSequence[line.querySeq];
				line.reverse = (t.name[qf] < 0) != (t.name[a.mate[qf]] < 0);
				line.queryBegin = t.begin[qf];
				line.queryEnd = uint64_t(t.end[ql]) + k;
				line.refBegin = t.begin[rf];
				line.refEnd = uint64_t(t.end[rl]) + k;
				line.anchors = uint64_t(ql) - qf + 1;
				return line;
			}
		}

		void WriteAnchors(const EventTable & t, size_t k, const ColorMap & map, const InputSequences & seq, const AnchorTable & a, const std::string & path)
		{
			CheckAnchors(t, map, seq, a);
			WriteStreamed(path, "anchor table", [&](std::string & buf, const std::function<void()> & flushIfLarge)
			{
				buf += "#twopaco-anchors\t1\tby=" + std::string(map.bySequence ? "sequence" : "file") + "\tk=" + std::to_string(k) + "\tcolors=" + std::to_string(a.colors) +
					"\tsegments=" + std::to_string(a.segments) + "\tref=" + std::to_string(a.ref) + "\tref_edges=" + std::to_string(a.refEdges) + "\tblocks=" +
					std::to_string(a.Rows()) + "\n";
				for (uint64_t c = 0; c < a.colors; c++) buf += "#color\t" + std::to_string(c) + "\t" + map.label[c] + "\n";
				for (size_t s = 0; s < seq.name.size(); s++)
				{
					buf += "#sequence\t" + std::to_string(s) + "\t" + std::to_string(map.colorOfSequence[s]) + "\t" + std::to_string(seq.length[s]) + "\t" + seq.name[s] + "\n";
					flushIfLarge();
				}

				for (uint64_t c = 0; c < a.colors; c++)
				{
					if (c == a.ref) continue;
					buf += "#shared\t" + std::to_string(c) + "\t" + std::to_string(a.blocks[c]) + "\t" + std::to_string(a.anchors[c]) + "\t" + std::to_string(a.edges[c]) + "\t" +
						std::to_string(a.reverseEdges[c]) + "\n";
				}

				for (size_t b = 0; b < a.Rows(); b++)
				{
					const AnchorLine line = MakeAnchorLine(t, k, map, a, b);
					buf += std::to_string(line.color) + "\t" + std::to_string(line.refSeq) + "\t" + std::to_string(line.refBegin) + "\t" + std::to_string(line.refEnd) + "\t" +
						(line.reverse ? "-" : "+") + "\t" + std::to_string(line.querySeq) + "\t" + std::to_string(line.queryBegin) + "\t" + std::to_string(line.queryEnd) + "\t" +
						std::to_string(line.anchors) + "\n";
					flushIfLarge();
				}
			});
		}

		void WriteAnchorsPaf(const EventTable & t, size_t k, const ColorMap & map, const InputSequences & seq, const AnchorTable & a, const std::string & path)
		{
			CheckAnchors(t, map, seq, a);
			if (path.empty()) throw std::runtime_error("The anchor PAF needs a file name");
			WriteStreamed(path, "anchor PAF", [&](std::string & buf, const std::function<void()> & flushIfLarge)
			{
				for (size_t b = 0; b < a.Rows(); b++)
				{
					const AnchorLine line = MakeAnchorLine(t, k, map, a, b);
					const std::string length = std::to_string(line.queryEnd - line.queryBegin);
					buf += seq.name[line.querySeq] + "\t" + std::to_string(seq.length[line.querySeq]) + "\t" + std::to_string(line.queryBegin) + "\t" + std::to_string(line.queryEnd) + "\t" +
						(line.reverse ? "-" : "+") + "\t" + seq.name[line.refSeq] + "\t" + std::to_string(seq.length[line.refSeq]) + "\t" + std::to_string(line.refBegin) + "\t" +
						std::to_string(line.refEnd) + "\t" + length + "\t" + length + "\t255\ttp:A:P\tcg:Z:" + length + "=\tan:i:" + std::to_string(line.anchors) + "\n";
					flushIfLarge();
				}
			});
		}

		void WriteAnchorFiles(const EventTable & t, size_t k, const ColorMap & map, const InputSequences & seq, const AnchorTable & a, const std::string & path,
			const std::string & pafPath)
		{
			if (!pafPath.empty()) WriteAnchorsPaf(t, k, map, seq, a, pafPath);
			try
			{
				WriteAnchors(t, k, map, seq, a, path);
			}
			catch (...)
			{
				if (!pafPath.empty()) ::unlink(pafPath.c_str());
				throw;
			}
		}

		namespace
		{
			char LocateLetter(char ch)
			{
				return ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T' ? ch : 'N';
			}

			std::string ReverseComplement(const std::string & w)
			{
				std::string r(w.rbegin(), w.rend());
				for (char & ch : r) ch = ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : 'N';
				return r;
			}

			void CheckLocate(const ColorMap & map, size_t queries, const LocateTable & l)
			{
				const size_t runs = l.Runs();
				if (l.found.size() != queries || l.forward.size() != queries || l.runs.size() != queries || l.windows.size() != queries || l.shared.size() != queries * l.colors ||
					map.label.size() != l.colors || l.runBegin.size() != runs || l.runLength.size() != runs || l.runRow.size() != runs || l.runRev.size() != runs || l.runOff.size() != runs)
				{
					throw std::runtime_error("locate table: the arrays do not agree about the queries, the runs and the colours");
				}
			}
		}

		void BuildEdgeIndex(const EventTable & t, const LoadedSequences & loaded, size_t k, EdgeIndex & out)
		{
			if (loaded.body.size() != t.sequences) throw std::runtime_error("edge index: the letters of every sequence are required");
			if (!t.seqEventBegin || t.seqEventBegin[0] != 0 || t.seqEventBegin[t.sequences] != t.events) throw std::runtime_error("event table: the sequences' event ranges do not cover the events");
			out = EdgeIndex();
			out.k = k;
			const size_t n = k + 1;
			std::vector<uint64_t> start;
			out.text = "N";
			for (const std::string & body : loaded.body)
			{
				start.push_back(out.text.size());
				for (char ch : body) out.text += LocateLetter(ch);
				out.text += 'N';
			}

			size_t sequence = 0;
			for (uint64_t e = 0; e < t.events; e++)
			{
				while (e >= t.seqEventBegin[sequence + 1]) ++sequence;
				if (!((t.first[e >> 5] >> (e & 31)) & 1u)) continue;
				if (t.end[e] < t.begin[e] || t.end[e] > loaded.body[sequence].size()) throw std::runtime_error("edge index: an event lies outside its sequence");
				const uint32_t row = uint32_t(out.g0.size());
				const uint64_t g0 = start[sequence] + t.begin[e];
				out.g0.push_back(g0);
				for (uint64_t g = g0; g < g0 + (t.end[e] - t.begin[e]); g++)
				{
					if (g + n > out.text.size()) { ++out.skipped; continue; }
					std::string w = out.text.substr(size_t(g), n);
					if (w.find('N') != std::string::npos) { ++out.skipped; continue; }
					const std::string r = ReverseComplement(w);
					if (r < w) w = r;
					auto seen = out.entry.find(w);
					if (seen == out.entry.end()) out.entry.emplace(w, std::make_pair(g, row));
					else
					{
						++out.duplicates;
						if (g < seen->second.first) seen->second = std::make_pair(g, row);
					}
				}
			}
		}

		void ComputeLocate(const EdgeIndex & index, const ColorTable & colors, const LoadedSequences & queries, LocateTable & out)
		{
			if (colors.Rows() != index.g0.size()) throw std::runtime_error("locate table: the colour table and the edge index disagree about the segments");
			out = LocateTable();
			out.colors = colors.colors;
			out.segments = index.g0.size();
			out.entries = index.entry.size();
			out.duplicates = index.duplicates;
			const size_t n = index.k + 1, words = colors.Words(), records = queries.body.size();
			out.windows.assign(records, 0);
			out.found.assign(records, 0);
			out.forward.assign(records, 0);
			out.runs.assign(records, 0);
			out.shared.assign(records * size_t(out.colors), 0);
			for (size_t q = 0; q < records; q++)
			{
				std::string body;
				for (char ch : queries.body[q]) body += LocateLetter(ch);
				bool open = false;           // the window before this one was a hit: (row, rev, off) below are its
				uint32_t lastRow = 0, lastRev = 0;
				uint64_t lastOff = 0;
				for (size_t p = 0; p + n <= body.size(); p++)
				{
					const std::string w = body.substr(p, n);
					if (w.find('N') != std::string::npos) { open = false; continue; }
					++out.windows[q];
					const std::string r = ReverseComplement(w);
					auto seen = index.entry.find(r < w ? r : w);
					if (seen == index.entry.end()) { open = false; continue; }
					const uint64_t g = seen->second.first;
					const uint32_t row = seen->second.second;
					const uint32_t rev = index.text.compare(size_t(g), n, w) == 0 ? 0u : 1u;
					const uint64_t off = g - index.g0[row];
					++out.found[q];
					if (!rev) ++out.forward[q];
					for (uint64_t c = 0; c < out.colors; c++)
					{
						if ((colors.presence[size_t(row) * words + size_t(c >> 5)] >> (c & 31)) & 1u) ++out.shared[q * size_t(out.colors) + size_t(c)];
					}

					if (open && row == lastRow && rev == lastRev && (rev ? off + 1 == lastOff : off == lastOff + 1)) ++out.runLength.back();
					else
					{
						++out.runs[q];
						out.runQuery.push_back(q);
						out.runBegin.push_back(p);
						out.runLength.push_back(1);
						out.runRow.push_back(row);
						out.runRev.push_back(rev);
						out.runOff.push_back(uint32_t(off));
					}

					open = true;
					lastRow = row;
					lastRev = rev;
					lastOff = off;
				}
			}
		}

		void WriteLocate(size_t k, const ColorMap & map, const InputSequences & queries, const LocateTable & l, const std::string & path)
		{
			CheckLocate(map, queries.name.size(), l);
			if (queries.length.size() != queries.name.size()) throw std::runtime_error("locate table: the name and the length of every query are required");
			WriteStreamed(path, "locate table", [&](std::string & buf, const std::function<void()> & flushIfLarge)
			{
				buf += "#twopaco-locate\t1\tby=" + std::string(map.bySequence ? "sequence" : "file") + "\tk=" + std::to_string(k) + "\tcolors=" + std::to_string(l.colors) +
					"\tsegments=" + std::to_string(l.segments) + "\tentries=" + std::to_string(l.entries) + "\tduplicates=" + std::to_string(l.duplicates) + "\tqueries=" +
					std::to_string(l.Queries()) + "\n";
				for (uint64_t c = 0; c < l.colors; c++) buf += "#color\t" + std::to_string(c) + "\t" + map.label[c] + "\n";
				uint64_t total[4] = {0, 0, 0, 0};
				for (size_t q = 0; q < l.Queries(); q++)
				{
					buf += queries.name[q] + "\t" + std::to_string(queries.length[q]) + "\t" + std::to_string(l.windows[q]) + "\t" + std::to_string(l.found[q]) + "\t" +
						std::to_string(l.forward[q]) + "\t" + std::to_string(l.runs[q]);
					for (uint64_t c = 0; c < l.colors; c++) buf += "\t" + std::to_string(l.shared[q * size_t(l.colors) + size_t(c)]);
					buf += "\n";
					total[0] += l.windows[q]; total[1] += l.found[q]; total[2] += l.forward[q]; total[3] += l.runs[q];
					flushIfLarge();
				}

				buf += "#total\t" + std::to_string(total[0]) + "\t" + std::to_string(total[1]) + "\t" + std::to_string(total[2]) + "\t" + std::to_string(total[3]) + "\n";
			});
		}

		void WriteLocateWalks(const EventTable & t, size_t k, const ColorTable & colors, const LocateTable & l, const std::string & path)
		{
			if (path.empty()) throw std::runtime_error("The locate walks need a file name");
			for (size_t i = 0; i < l.Runs(); i++)
			{
				if (l.runRow[i] >= colors.Rows() || colors.firstEvent[l.runRow[i]] >= t.events) throw std::runtime_error("locate table: a run lies outside the segments");
			}

			WriteStreamed(path, "locate walks", [&](std::string & buf, const std::function<void()> & flushIfLarge)
			{
				buf += "#twopaco-locate-walks\t1\tk=" + std::to_string(k) + "\n";
				for (size_t i = 0; i < l.Runs(); i++)
				{
					const uint32_t e0 = colors.firstEvent[l.runRow[i]];
					const uint64_t length = l.runLength[i], body = uint64_t(t.end[e0]) - t.begin[e0] + k;
					// the span's letters the run covers, in text orientation
					uint64_t sBegin = l.runRev[i] ? uint64_t(l.runOff[i]) + 1 - length : uint64_t(l.runOff[i]), sEnd = sBegin + length + k;
					bool minus = l.runRev[i] != 0;
					if (t.name[e0] < 0)
					{
						const uint64_t b = body - sEnd;
						sEnd = body - sBegin;
						sBegin = b;
						minus = !minus;
					}

					buf += std::to_string(l.runQuery[i]) + "\t" + std::to_string(l.runBegin[i]) + "\t" + std::to_string(l.runBegin[i] + length + k) + "\t" +
						std::to_string(static_cast<long long>(Magnitude(t.name[e0]))) + "\t" + (minus ? "-" : "+") + "\t" + std::to_string(sBegin) + "\t" + std::to_string(sEnd) + "\n";
					flushIfLarge();
				}
			});
		}

		void WriteLocateFiles(const EventTable & t, size_t k, const ColorMap & map, const ColorTable & colors, const InputSequences & queries, const LocateTable & l,
			const std::string & path, const std::string & walksPath)
		{
			CheckLocate(map, queries.name.size(), l);
			if (!walksPath.empty()) WriteLocateWalks(t, k, colors, l, walksPath);
			try
			{
				WriteLocate(k, map, queries, l, path);
			}
			catch (...)
			{
				if (!walksPath.empty()) ::unlink(walksPath.c_str());
				throw;
			}
		}

		void WriteGraphFile(const EventTable & table, const InputSequences & seq, const LoadedSequences & loaded, size_t k, const std::string & format,
			size_t threads, const std::string & outPath)
		{
			WriteGraphFileWith(format, seq, outPath, [&](int fd, uint64_t fileOffset)
			{
				return FormatEvents(table, seq, loaded, k, format, threads, fd, fileOffset);
			}, format == "gfa1" && table.linkFirst != 0);
		}
	}
}
