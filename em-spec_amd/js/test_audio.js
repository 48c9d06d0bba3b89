// The live audio history through the addon (engine.setLiveAudio / liveAudio / audioView / reanalyse), for
// tests/test_gpu_live_audio_node.py:
//   node test_audio.js <feed.f32> <out.bin> S L fftSize hop rows W
// feed: float32 [S][L].  One EXACT session: one computeSpectrogramColumns call per hop; after every call liveAudio must give
// the samples stored so far and the first one held.  Then the view of everything held must be the samples fed, bit for bit, and
// reanalyse of it at fftSize 256 / hop 128 must be computeColumns of those samples, byte for byte; the view, the re-analysis' dB
// and its index bytes are appended to out.bin - the Python test holds them against its own binding's.  Prints one JSON line.
'use strict';
const fs = require('fs');
const em = require('./index.js');

const [feedPath, outPath] = process.argv.slice(2, 4);
const [S, L, fftSize, hop, rows, W] = process.argv.slice(4, 10).map(Number);
const raw = fs.readFileSync(feedPath);
const pcm = new Float32Array(raw.buffer, raw.byteOffset, raw.length / 4);
if (pcm.length !== S * L) throw new Error(`feed holds ${pcm.length} samples, not ${S * L}`);
const same = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;

const engine = em.createEngine({ streams: S, rows, exact: true });
if (engine.liveAudio(0) !== null) throw new Error('an audio history before it is set');
engine.setLiveAudio(W);
const hops = (L - fftSize) / hop + 1;
const frames = new Float32Array(S * fftSize);
for (let j = 0; j < hops; j++) {
  for (let s = 0; s < S; s++) frames.set(pcm.subarray(s * L + j * hop, s * L + j * hop + fftSize), s * fftSize);
  engine.computeSpectrogramColumns(frames, fftSize, hop, true);
  const end = j * hop + fftSize;
  for (let s = 0; s < S; s++) {
    const h = engine.liveAudio(s);
    if (!h || h.end !== end || h.first !== Math.max(0, end - W)) throw new Error(`hop ${j}: stream ${s} holds ${JSON.stringify(h)}, fed ${end}`);
  }
}
const { end, first } = engine.liveAudio(0);
const count = end - first;
const view = engine.audioView({ firstSample: first, count });
const fed = new Float32Array(S * count);
for (let s = 0; s < S; s++) fed.set(pcm.subarray(s * L + first, s * L + end), s * count);
if (!same(new Uint32Array(view.buffer), new Uint32Array(fed.buffer))) throw new Error('the view is not the samples fed');
const part = engine.audioView({ stream0: 1, streams: 1, firstSample: end - 7, count: 7 });
if (!same(part, pcm.subarray(L + end - 7, L + end))) throw new Error('the view of one stream is not the samples fed');

const re = engine.reanalyse({ firstSample: first, count, fftSize: 256, hop: 128, reassign: false, want: ['db', 'index', 'rgba'] });
const C = em.numColumns(count, 256, 128);
if (re.columns !== C) throw new Error(`reanalyse returned ${re.columns} columns, not ${C}`);
const ref = { db: new Float32Array(S * C * rows), rgba: new Uint8Array(4 * S * C * rows), index: new Uint8Array(S * C * rows) };
engine.computeColumns(fed, S, count, 256, 128, false, ref);
if (!same(re.db, ref.db) || !same(re.index, ref.index) || !same(re.rgba, ref.rgba)) throw new Error('reanalyse is not computeColumns of the samples');
fs.writeFileSync(outPath, Buffer.concat([view, re.db, re.index].map((a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength))));

// the session goes on behind a re-analysis; refusals leave the engine usable
engine.computeSpectrogramColumns(frames, fftSize, hop, true);
if (engine.liveAudio(0).end !== end + hop) throw new Error('the session did not go on');
let code = 'none';
try { engine.audioView({ firstSample: engine.liveAudio(0).first - 1, count: 2 }); } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_INVALID_ARG') throw new Error(`a view below the held range gave ${code}`);
try { engine.reanalyse({ firstSample: engine.liveAudio(0).first, count: 100, fftSize: 256, hop: 128 }); code = 'none'; } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_INVALID_ARG') throw new Error(`a re-analysis of fewer samples than a frame gave ${code}`);
try { engine.setLiveAudio(W); code = 'none'; } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_STATE') throw new Error(`setLiveAudio mid-session gave ${code}`);
if (engine.audioView({ firstSample: engine.liveAudio(0).first, count: 1 }).length !== S) throw new Error('a view after the refusals');
engine.setLiveAudio(0);
if (engine.liveAudio(0) !== null) throw new Error('a cleared audio history still answers');
try { engine.audioView({ firstSample: 0, count: 1 }); code = 'none'; } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_STATE') throw new Error(`a view without an audio history gave ${code}`);
engine.destroy();
console.log(JSON.stringify({ ok: true, S, hops, W, end, first, columns: C }));
