"""Rate control: a sequence coded to a target bitrate, one q_index per closed GOP.

Closed GOPs are coded independently into their own folders (pmctf_seq) and the exact size of a coding is the size of its
files, so the controller needs no model of the coder: it codes a GOP at a q_index, looks at the files, and moves at most
a few steps up or down the list of choices.  A leaky bucket carries what a GOP leaves of its share to the GOPs after it.
  gop_allocations, choose_q, run_controller   the controller: pure Python, exact in integers (bits), no torch
  encode_sequence_rate                        pmctf_seq.encode_sequence_gops with bitrate and fps instead of q_index:
                                              every trial is pmctf_gop.encode_gop / encode_lone_picture, the HIP path
  verify_rate_record                          rate_control.json against the files and the header: no GPU, no codec
The folder's gop_structure.json is format version 2 (a q_index in every GOP entry), which the decoders read.  Nothing
here has a CPU path for the coding itself, and nothing here computes on pictures."""
import os

from pmctf_records import is_int, read_record, write_record

RATE_RECORD = "rate_control.json"
RATE_RECORD_VERSION = 1
Q_NUM = 21                                            # pWave.get_qp_num(): q_index is one of 0..20
RECORD_FIELDS = ("alloc", "budget", "q_index", "fits", "bits", "trials", "credit")
PARAMETERS = ("bitrate", "fps", "q_choices", "q_start", "bucket_ms", "max_trials", "slack")


def trial_folder(k, q):
    """sub-folder of GOP k's trial at q_index q while encode_sequence_rate is choosing"""
    return f"gop_{k:05d}.q{q:02d}.trial"


# ---------------------------------------------------------------------------------------------------------- the arguments
def check_bitrate(bitrate):
    if not is_int(bitrate) or bitrate <= 0:
        raise ValueError(f"bitrate is a positive integer, in bits per second (got {bitrate!r})")
    return bitrate


def check_fps(fps):
    """-> (num, den) of fps: a positive integer, or a pair (num, den) of positive integers"""
    if is_int(fps):
        fps = (fps, 1)
    if not isinstance(fps, (tuple, list)) or len(fps) != 2 or not all(is_int(v) and v > 0 for v in fps):
        raise ValueError(f"fps is a positive integer or a pair (num, den) of positive integers (got {fps!r})")
    return int(fps[0]), int(fps[1])


def check_q_choices(q_choices):
    """-> q_choices as a tuple: strictly ascending integers of 0..20, at least one"""
    try:
        q = tuple(q_choices)
    except TypeError:
        q = None
    if not q or not all(is_int(v) and 0 <= v < Q_NUM for v in q) or any(a >= b for a, b in zip(q, q[1:])):
        raise ValueError(f"q_choices is a strictly ascending sequence of integers of 0..{Q_NUM - 1} (got {q_choices!r})")
    return q


def check_max_trials(max_trials):
    if not is_int(max_trials) or max_trials < 1:
        raise ValueError(f"max_trials is an integer, at least 1 (got {max_trials!r})")
    return max_trials


def check_slack(slack):
    if isinstance(slack, bool) or not isinstance(slack, (int, float)) or not 0 <= slack < 1:
        raise ValueError(f"slack is a number in [0, 1) (got {slack!r})")
    return slack


def check_bucket_ms(bucket_ms):
    if not is_int(bucket_ms) or bucket_ms < 0:
        raise ValueError(f"bucket_ms is an integer, 0 or more, in milliseconds (got {bucket_ms!r})")
    return bucket_ms


def check_q_start(q_start, q_choices):
    """-> the index of q_start in q_choices; None: the middle one, q_choices[len // 2]"""
    if q_start is None:
        return len(q_choices) // 2
    if not is_int(q_start) or q_start not in q_choices:
        raise ValueError(f"q_start is one of q_choices {tuple(q_choices)} (got {q_start!r})")
    return q_choices.index(q_start)


# --------------------------------------------------------------------------------------------------------- the controller
def gop_allocations(gops, bitrate, fps):
    """-> alloc[k] = (size_k * bitrate * den) // num: the bits GOP k's pictures last at `bitrate` bits per second and
    fps = num / den pictures per second, rounded down.  gops: a list of {"first", "size", ...}."""
    check_bitrate(bitrate)
    num, den = check_fps(fps)
    out = []
    try:
        sizes = [g["size"] for g in gops]
    except (TypeError, KeyError, IndexError):
        raise ValueError(f"gops is a list of records that hold \"size\" (got {gops!r})") from None
    for k, size in enumerate(sizes):
        if not is_int(size) or size < 1:
            raise ValueError(f"gops[{k}]: size is a positive integer (got {size!r})")
        out.append((size * bitrate * den) // num)
    return out


def choose_q(size_of, q_choices, start, budget, max_trials=4, slack=0.0):
    """One GOP's q_index.  size_of(q) -> the bits of the GOP coded at q: called at most once per q and at most max_trials
    times.  Nothing is assumed about how the size depends on q; the result is what these steps give:
      1. try q_choices[start];
      2. it fits (bits <= budget): climb.  While a higher index exists, trials are left and the best fitting trial has
         bits < (1 - slack) * budget, try the next index; a trial that fits becomes the best, one that does not ends the
         climb.  The best is accepted, fits=True;
      3. it does not fit: descend.  While a lower index exists and trials are left, try the next lower index; the first
         that fits is accepted, fits=True; when none does, the last one tried, fits=False.
    The accepted trial is the last one run or the one before it.
    -> {"q_index", "index", "fits", "bits", "trials": [(q, bits), ...] in the order run}"""
    q_choices = check_q_choices(q_choices)
    if not is_int(start) or not 0 <= start < len(q_choices):
        raise ValueError(f"start is an index into the {len(q_choices)} q_choices (got {start!r})")
    if not is_int(budget):
        raise ValueError(f"budget is an integer, in bits (got {budget!r})")
    check_max_trials(max_trials)
    check_slack(slack)
    trials = []

    def run(index):
        bits = size_of(q_choices[index])
        if not is_int(bits) or bits < 0:
            raise ValueError(f"size_of({q_choices[index]}) is a count of bits (got {bits!r})")
        trials.append((q_choices[index], bits))
        return bits

    index, bits = start, run(start)
    fits = bits <= budget
    if fits:
        while index + 1 < len(q_choices) and len(trials) < max_trials and bits < (1 - slack) * budget:
            more = run(index + 1)
            if more > budget:
                break
            index, bits = index + 1, more
    else:
        while not fits and index > 0 and len(trials) < max_trials:
            index, bits = index - 1, run(index - 1)
            fits = bits <= budget
    return {"q_index": q_choices[index], "index": index, "fits": fits, "bits": bits, "trials": trials}


class Controller:
    """run_controller, GOP by GOP, for a caller that learns the GOPs one at a time (encode_sequence_rate): budget(size),
    then gop(size, size_of) -> the GOP's record.  credit: what the GOPs so far left of their shares, at most bucket_bits."""

    def __init__(self, bitrate, fps, q_choices=range(Q_NUM), q_start=None, bucket_ms=1000, max_trials=4, slack=0.0):
        self.bitrate = check_bitrate(bitrate)
        self.fps = check_fps(fps)
        self.q_choices = check_q_choices(q_choices)
        self.index = check_q_start(q_start, self.q_choices)
        self.q_start = self.q_choices[self.index]
        self.bucket_ms = check_bucket_ms(bucket_ms)
        self.max_trials = check_max_trials(max_trials)
        self.slack = check_slack(slack)
        self.bucket_bits = (self.bitrate * self.bucket_ms) // 1000
        self.credit = 0

    def parameters(self):
        return {"bitrate": self.bitrate, "fps": list(self.fps), "q_choices": list(self.q_choices), "q_start": self.q_start,
                "bucket_ms": self.bucket_ms, "max_trials": self.max_trials, "slack": self.slack}

    def alloc(self, size):
        return (size * self.bitrate * self.fps[1]) // self.fps[0]

    def budget(self, size):
        """the next GOP's budget: its share plus the credit carried to it"""
        return self.alloc(size) + self.credit

    def gop(self, size, size_of):
        alloc, budget = self.alloc(size), self.budget(size)
        c = choose_q(size_of, self.q_choices, self.index, budget, self.max_trials, self.slack)
        self.index = c["index"]
        self.credit = min(self.bucket_bits, self.credit + alloc - c["bits"])
        return {"alloc": alloc, "budget": budget, "q_index": c["q_index"], "fits": c["fits"], "bits": c["bits"],
                "trials": c["trials"], "credit": self.credit}


def run_controller(gop_sizes, size_of, bitrate, fps, q_choices=range(Q_NUM), q_start=None, bucket_ms=1000, max_trials=4,
                   slack=0.0):
    """The q_index of every GOP of a sequence.  gop_sizes: pictures per GOP; size_of(k, q) -> the bits of GOP k at q.
    bucket_bits = (bitrate * bucket_ms) // 1000; credit starts at 0; for GOP k
      budget_k = alloc_k + credit                          (alloc: gop_allocations)
      choose_q from the index accepted for GOP k - 1       (GOP 0: from q_start, by default q_choices[len // 2])
      credit = min(bucket_bits, credit + alloc_k - bits_k)
    While every GOP fits, credit >= 0 and every prefix has sum(bits) <= sum(alloc): a GOP spends at most its share and
    what the GOPs before it left; the bucket only ever forgets credit.  A GOP that does not fit at the lowest choice
    tried takes the credit below 0, which the GOPs after it pay back.
    -> per GOP {"alloc", "budget", "q_index", "fits", "bits", "trials", "credit": after the GOP}"""
    ctl = Controller(bitrate, fps, q_choices, q_start, bucket_ms, max_trials, slack)
    sizes = list(gop_sizes)
    for k, size in enumerate(sizes):
        if not is_int(size) or size < 1:
            raise ValueError(f"gop_sizes[{k}] is a positive integer (got {size!r})")
    return [ctl.gop(size, lambda q, k=k: size_of(k, q)) for k, size in enumerate(sizes)]


# ------------------------------------------------------------------------------------------------------------ the encoder
def encode_sequence_rate(codec, source, width, height, frame_num, max_gop, bitrate, fps, bin_folder, device,
                         structure="fill", hd_min=None, mad_min=None, ds_factors=(1, 2, 4, 8), skip_decoding=True, psize=128,
                         src_format="yuv", ingest="host", decoded_frame_path=None, picture_hash=None, bitdepth=8,
                         msssim=False, q_choices=range(Q_NUM), q_start=None, bucket_ms=1000, max_trials=4, slack=0.0):
    """pmctf_seq.encode_sequence_gops at `bitrate` bits per second for a source of `fps` pictures per second (an integer or
    (num, den)) instead of at one q_index: run_controller (whose keywords are the last five) decides GOP k's q_index from
    codings of the GOP itself.  structure: "fill", "scenecut" or an explicit list; "search" is refused (it ranks GOP
    sizes at one fixed q_index).  hd_min, mad_min: None for pmctf_seq's defaults.  Everything else is
    encode_sequence_gops', and the loop over the GOPs is the very same code.
    Every trial of GOP k is pmctf_gop.encode_gop (a lone picture: codec.encode_lone_picture) at q into
    bin_folder/gop_{k:05d}.q{q:02d}.trial/; its size is 8 x the sizes of pmctf_gop.gop_file_names(size) there (a lone
    picture: of its two L files).  At any time only the best fitting trial so far and the newest one are kept, as folders
    and as results.  The accepted trial, always one of those two, is renamed to gop_{k:05d} (a folder of that name from an
    earlier run is replaced) and the other removed, whatever happens (try / finally); the reconstruction, quality, hashes
    and PNGs of a GOP are the accepted trial's, computed once.
    bin_folder gets the version-2 gop_structure.json and rate_control.json: {"format_version": 1, the parameters,
    "bucket_bits", "gops": run_controller's records}; verify_rate_record checks it.
    Returns encode_sequence_gops' dictionary ("gops" with each GOP's "q_index"; the "average ms" lines count accepted
    trials only) plus "rate": run_controller's records, each with "seconds", the wall time of all the GOP's trials."""
    return _encode_at_rate(codec, source, width, height, frame_num, max_gop, bitrate, fps, bin_folder, device,
                           structure=structure, hd_min=hd_min, mad_min=mad_min, ds_factors=ds_factors,
                           skip_decoding=skip_decoding, psize=psize, src_format=src_format, ingest=ingest,
                           decoded_frame_path=decoded_frame_path, picture_hash=picture_hash, bitdepth=bitdepth, msssim=msssim,
                           q_choices=q_choices, q_start=q_start, bucket_ms=bucket_ms, max_trials=max_trials, slack=slack)


def _encode_at_rate(codec, source, width, height, frame_num, max_gop, bitrate, fps, bin_folder, device, *, pipeline=None,
                    **options):
    """encode_sequence_rate's body.  options: the controller's keywords (PARAMETERS) and those of pmctf_seq's GOP-list
    body; pipeline: a pmctf_chroma.SourcePipeline or None."""
    import shutil
    import pmctf_gop
    import pmctf_seq
    ctl = Controller(bitrate, fps, **{k: options.pop(k) for k in PARAMETERS[2:] if k in options})
    if options.get("structure") == "search":
        raise ValueError("structure 'search' is refused with a bitrate: it ranks GOP sizes at one fixed q_index")
    records = []
    made = set()                                      # the trial folders of this call that still exist

    def drop(t):
        if t["folder"] in made:
            shutil.rmtree(t["folder"], ignore_errors=True)
            made.discard(t["folder"])

    def choose(k, g, trial):
        best = last = None                            # the best fitting trial so far, the newest trial: all that is kept
        budget = ctl.budget(g["size"])
        spent = 0.0

        def size_of(q):
            nonlocal best, last, spent
            if last is not None and last is not best:
                drop(last)
            last = None
            folder = os.path.join(bin_folder, trial_folder(k, q))
            made.add(folder)
            last = trial(q, folder)
            spent += last["seconds"]
            if last["bits"] <= budget:
                if best is not None:
                    drop(best)
                best = last
            return last["bits"]

        try:
            rec = ctl.gop(g["size"], size_of)
            accepted = best if rec["fits"] else last
            assert accepted["q_index"] == rec["q_index"] and accepted["bits"] == rec["bits"] and rec["budget"] == budget
            final = os.path.join(bin_folder, pmctf_gop.gop_folder(k))
            if os.path.isdir(final):
                shutil.rmtree(final)
            os.rename(accepted["folder"], final)
            made.discard(accepted["folder"])
            accepted["folder"] = final
        finally:
            for t in (best, last):
                if t is not None:
                    drop(t)
            for folder in sorted(made):
                shutil.rmtree(folder, ignore_errors=True)
            made.clear()
        records.append(dict(rec, seconds=spent))
        return accepted

    for k, default in (("hd_min", pmctf_seq.HD_MIN), ("mad_min", pmctf_seq.MAD_MIN)):
        if options.get(k) is None:
            options[k] = default
    out = pmctf_seq._encode_gop_list(codec, source, width, height, frame_num, max_gop, None, bin_folder, device,
                                     choose=choose, pipeline=pipeline, what="encode_sequence_rate", **options)
    write_rate_record(bin_folder, ctl, [{f: r[f] for f in RECORD_FIELDS} for r in records])
    out["rate"] = records
    return out


# ------------------------------------------------------------------------------------------------------------- the record
def write_rate_record(bin_folder, ctl, records):
    """bin_folder/rate_control.json: format version, the controller's parameters, bucket_bits and one record per GOP"""
    path = os.path.join(bin_folder, RATE_RECORD)
    record = dict(ctl.parameters(), format_version=RATE_RECORD_VERSION, bucket_bits=ctl.bucket_bits,
                  gops=[dict(r, trials=[list(t) for t in r["trials"]]) for r in records])
    return write_record(path, record, indent=1)


def read_rate_record(bin_folder):
    """-> the record of bin_folder/rate_control.json with its fields checked for form (verify_rate_record checks what
    they say); ValueError naming the path for a missing or malformed file, another version, unknown or missing fields"""
    path = os.path.join(bin_folder, RATE_RECORD)
    record = read_record(path, "rate control record", RATE_RECORD_VERSION, fields=PARAMETERS + ("bucket_bits", "gops"),
                         missing="not a folder written with encode_sequence_rate", reader="checker")
    try:
        ctl = Controller(*(record[k] for k in PARAMETERS))
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None
    if record["bucket_bits"] != ctl.bucket_bits:
        raise ValueError(f"{path}: bucket_bits {record['bucket_bits']!r}, bitrate and bucket_ms give {ctl.bucket_bits}")
    if not isinstance(record["gops"], list):
        raise ValueError(f"{path}: gops is a list")
    for k, r in enumerate(record["gops"]):
        if not isinstance(r, dict) or set(r) != set(RECORD_FIELDS):
            raise ValueError(f"{path}: gops[{k}] holds exactly {RECORD_FIELDS}")
        if not all(is_int(r[f]) for f in ("alloc", "budget", "q_index", "bits", "credit")) or not isinstance(r["fits"], bool):
            raise ValueError(f"{path}: gops[{k}]: alloc, budget, q_index, bits and credit are integers, fits is true or false")
        if not isinstance(r["trials"], list) or not r["trials"] or not all(
                isinstance(t, list) and len(t) == 2 and all(is_int(v) for v in t) for t in r["trials"]):
            raise ValueError(f"{path}: gops[{k}]: trials is a non-empty list of [q_index, bits]")
    return record


def verify_rate_record(bin_folder):
    """rate_control.json against the folder it lies in, with no GPU and no codec: every accepted size recomputed from the
    files on disk (8 x the sizes of pmctf_gop.gop_file_names(size) in gop_{k:05d}/), the credit arithmetic replayed from
    the parameters, every `fits` against bits <= budget, the accepted trial among the GOP's trials, and the header's
    per-GOP q_index against the record's.  ValueError naming the path and the first violation.
    -> {"record", "header", "frame_num", "total_bits", "bits_per_second": total_bits * num / (den * frame_num), a float}"""
    import pmctf_gop
    import pmctf_seq
    path = os.path.join(bin_folder, RATE_RECORD)
    record = read_rate_record(bin_folder)
    header = pmctf_seq.read_gop_structure(bin_folder)
    if header["format_version"] != pmctf_gop.GOP_STRUCTURE_VERSION_Q:
        raise ValueError(f"{path}: {pmctf_gop.GOP_STRUCTURE} is format version {header['format_version']}: it holds no "
                         f"q_index per GOP")
    gops = header["gops"]
    if len(record["gops"]) != len(gops):
        raise ValueError(f"{path}: {len(record['gops'])} GOP records, the header lists {len(gops)} GOPs")
    ctl = Controller(*(record[k] for k in PARAMETERS))
    total = 0
    for k, (g, r) in enumerate(zip(gops, record["gops"])):
        where = f"{path}: GOP {k}"
        if r["q_index"] != g["q_index"]:
            raise ValueError(f"{where}: q_index {r['q_index']}, the header says {g['q_index']}")
        folder = os.path.join(bin_folder, pmctf_gop.gop_folder(k))
        bits = 0
        for name in (pmctf_gop.gop_file_names(g["size"]) if g["size"] > 1 else ("0_main.bin", "0_C_main.bin")):
            try:
                bits += 8 * os.path.getsize(os.path.join(folder, name))
            except OSError:
                raise ValueError(f"{where}: {os.path.join(folder, name)}: missing") from None
        if r["bits"] != bits:
            raise ValueError(f"{where}: bits {r['bits']}, the files in {folder} hold {bits}")
        alloc, budget = ctl.alloc(g["size"]), ctl.budget(g["size"])
        if r["alloc"] != alloc:
            raise ValueError(f"{where}: alloc {r['alloc']}, {g['size']} pictures at the bitrate get {alloc}")
        if r["budget"] != budget:
            raise ValueError(f"{where}: budget {r['budget']}, alloc {alloc} and the credit {ctl.credit} before it give {budget}")
        if r["fits"] != (bits <= budget):
            raise ValueError(f"{where}: fits {r['fits']}, but bits {bits} {'<=' if bits <= budget else '>'} budget {budget}")
        if r["q_index"] not in ctl.q_choices or [r["q_index"], bits] not in r["trials"][-2:]:
            raise ValueError(f"{where}: q_index {r['q_index']} at {bits} bits is not one of the last two trials "
                             f"{r['trials'][-2:]} of the choices {ctl.q_choices}")
        if len(r["trials"]) > ctl.max_trials:
            raise ValueError(f"{where}: {len(r['trials'])} trials, max_trials is {ctl.max_trials}")
        ctl.credit = min(ctl.bucket_bits, ctl.credit + alloc - bits)
        if r["credit"] != ctl.credit:
            raise ValueError(f"{where}: credit {r['credit']}, min(bucket_bits, credit + alloc - bits) gives {ctl.credit}")
        total += bits
    num, den = ctl.fps
    return {"record": record, "header": header, "frame_num": header["frame_num"], "total_bits": total,
            "bits_per_second": total * num / (den * header["frame_num"])}
