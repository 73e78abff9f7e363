"""BGZF members inflated on the device (csrc/kr_dev_bgzf.inc through kr_debug_bgzf_inflate): the kernel's bytes are zlib's for every
block type, size and member count of tests/bgzf_cases.py, and damaged members -- only those the decoder's host instantiation
rejected on the CPU (tests/test_bgzf_host.py) -- give KR_ERR_FORMAT naming the member, after which the stream inflates a good chunk."""
import pytest

import bgzf_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stream(capi, toy_index_dir):
    hx = capi.HostIndex(toy_index_dir)
    dx = hx.upload(0)
    st = dx.stream(capi.default_params(), max_reads=64, max_bases=4096)
    st.fastq_enable(1 << 20)
    st.bgzf_enable(1 << 20)
    yield st
    st.close()
    dx.close()
    hx.close()


@pytest.mark.parametrize("name", sorted(bc.corpus()))
def test_the_kernel_gives_zlibs_bytes(capi, stream, name):
    comp, want = bc.corpus()[name]
    assert stream.bgzf_inflate(comp) == want == capi.bgzf_inflate_host(comp)


def test_members_of_every_kind_in_one_call(capi, stream):
    cases = bc.corpus()
    names = [n for n in sorted(cases) if not n.startswith("members_")]
    comp = b"".join(cases[n][0] for n in names)
    assert stream.bgzf_inflate(comp) == b"".join(cases[n][1] for n in names)


@pytest.mark.parametrize("name", sorted(bc.damaged()))
def test_damaged_members_are_named_and_the_stream_goes_on(capi, stream, name):
    comp, words = bc.damaged()[name]
    good, text = bc.corpus()["members_5"]
    with pytest.raises(capi.KrError) as host:  # (first on the CPU: only what the host instantiation rejects reaches the kernel)
        capi.bgzf_inflate_host(good + comp + good)
    assert host.value.code == capi.KR_ERR_FORMAT and words in str(host.value)
    with pytest.raises(capi.KrError) as dev:
        stream.bgzf_inflate(good + comp + good)
    assert dev.value.code == capi.KR_ERR_FORMAT and str(dev.value) == str(host.value)
    assert "offset %d" % len(good) in str(dev.value)
    assert stream.bgzf_inflate(good) == text


def test_not_enabled_and_oversized_input_are_refused(capi, toy_index_dir):
    hx = capi.HostIndex(toy_index_dir)
    dx = hx.upload(0)
    st = dx.stream(capi.default_params(), max_reads=64, max_bases=4096)
    comp, text = bc.corpus()["members_4"]
    for call in (lambda: st.bgzf_enable(1 << 16), lambda: st.bgzf_inflate(comp), lambda: st.submit_bgzf(comp, 0, len(text))):
        with pytest.raises(capi.KrError) as e:
            call()
        assert e.value.code == capi.KR_ERR_STATE
    st.fastq_enable(1000)
    st.bgzf_enable(len(comp))
    with pytest.raises(capi.KrError) as e:
        st.bgzf_enable(len(comp))
    assert e.value.code == capi.KR_ERR_STATE
    with pytest.raises(capi.KrError) as e:
        st.bgzf_inflate(comp + bc.EOF_MEMBER)  # more compressed bytes than enabled for
    assert e.value.code == capi.KR_ERR_ARG
    with pytest.raises(capi.KrError) as e:
        st.bgzf_inflate(comp)  # more inflated bytes than kr_stream_fastq_enable's 1000
    assert e.value.code == capi.KR_ERR_ARG
    with pytest.raises(capi.KrError) as e:
        st.bgzf_inflate(comp[:-1])
    assert e.value.code == capi.KR_ERR_FORMAT
    st.close()
    dx.close()
    hx.close()
