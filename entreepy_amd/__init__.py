"""entreepy_amd -- MI355X-native (gfx950) Huffman encode/decode path for typio/entreepy.

The package is a thin host-side mirror of the reference's codec interface
(src/encode.zig:25, src/decode.zig:13) over libentreepy_hip.so, whose C ABI is
declared in include/entreepy_hip.h.  No CPU fallback exists.
"""
from .codec import (  # noqa: F401
    ASCII_LOWER,
    ASCII_UPPER,
    Codebook,
    Context,
    DecodeFlags,
    EmptyInputError,
    EncodeFlags,
    EntreepyError,
    FIELD_ABSENT,
    FIELD_TO_END,
    GROUP_NONE,
    GroupResult,
    JoinResult,
    MATCH_EQUAL,
    MATCH_LESS,
    MATCH_LESS_EQUAL,
    MATCH_NOT,
    MATCH_PREFIX,
    MatchResult,
    NUMBER_BAD,
    NUMBER_EMPTY,
    NUMBER_OK,
    NUMBER_RANGE,
    NumberResult,
    PackedResult,
    RECODE_DROP,
    SEARCH_CONTAINS,
    SEARCH_SUFFIX,
    SLICE_NO_STOP,
    SLICE_TO_END,
    TakeResult,
    byte_map,
    decode,
    default_context,
    encode,
    encode_bound,
    parse_header,
)

__version__ = "0.1.0"
